"""UltimateSDUpscale (LD.py:7400-8325), the reference's img2img: an ESRGAN upscale of the picture, a linear tile-by-tile redraw
(VAE-encode, a few denoise steps, VAE-decode) and a "Half Tile" seam-fix pass over the tile borders.

The reference does the image plumbing between the stages with PIL on the host, on the whole canvas, for every tile.  Here the canvas is a
device-resident uint8 batch for the whole run — one upload at the start, one download at the end — and the plumbing is the 8-bit image
kernels of image.hip (`ops.u8_*`), bit-identical to Pillow.  Only the small latents cross to the host, as KSampler2 already does.  This
module holds the geometry (pure Python) and the job loop (torch as device memory); it imports no PIL.

Behaviours of the reference that are mirrored on purpose:
  * the canvas is ceil(side * upscale_by / 8) * 8 (new_init, LD.py:8159-8176);
  * the upscale model is applied once per entry of get_factors (LD.py:7825-7863), whatever its own scale is, every time to every image
    of the batch; the result is Lanczos-resized to the canvas.  An `upscale_by` whose factor list would never terminate there (a scale
    factor of 5, 7, 10, ...) is a ValueError here;
  * a redraw tile is ceil((tile + padding) / 8) * 8 (new_setup_redraw, LD.py:8182-8189); a seam-fix tile is exactly tile_width x tile_height
    (half_tile_process sets p.width / p.height itself, LD.py:8016-8017), so with a seam fix those must be multiples of 8 (the VAE's stride);
  * ImageDraw.rectangle is inclusive, so the redraw mask is one pixel wider and higher than the tile (LD.py:7937-7952);
  * the seam-fix pass samples with `denoise`, NOT `seam_fix_denoise`: the reference stores the latter in p.denoising_strength, which
    process_images never reads (LD.py:8011, 7699);
  * `seam_fix_width` is unused (only the band-pass variant would read it);
  * a batch of B > 1 shares one crop per job and is encoded, sampled and decoded together (LD.py:7665-7707);
  * per job the host RNG is consumed in the reference's order: VAE.encode's posterior randn first, then prepare_noise's
    manual_seed(seed); every tile uses the same seed.
The reference runs its linear and half-tile loops for "Chess", "Band Pass" and "Half Tile + Intersections" too; those names are rejected
here rather than mislabel the result.
"""
from __future__ import annotations

import math
from types import SimpleNamespace
from typing import Optional

import torch

MODES = ("Linear", "Chess", "None")
SEAM_FIX_MODES = ("None", "Band Pass", "Half Tile", "Half Tile + Intersections")


# ------------------------------------------------------------------ geometry (pure Python)
def canvas_size(width: int, height: int, upscale_by: float):
    """(W, H) of the canvas: ceil(side * upscale_by / 8) * 8 (LD.py:8162-8163)."""
    return math.ceil((width * upscale_by) / 8) * 8, math.ceil((height * upscale_by) / 8) * 8


def get_factors(scale_factor: int):
    """USDUpscaler.get_factors (LD.py:7825-7845): the scale the reference THINKS each application of the upscale model has; the model is
    applied once per entry.  Where get_factor returns 0 the reference never terminates: ValueError."""
    def get_factor(num):
        if num == 1:
            return 2
        for f in (4, 3, 2):
            if num % f == 0:
                return f
        return 0
    scales, current = [], 1
    while current < scale_factor:
        f = get_factor(scale_factor // current)
        if f == 0:
            raise ValueError(f"upscale_by gives the scale factor {scale_factor}, for which the reference's get_factors never terminates "
                             f"(no factor 4, 3 or 2 of {scale_factor // current}); use a factor made of 2s, 3s and 4s")
        scales.append(f)
        current *= f
    return scales


def fix_crop_region(region, image_size):
    """LD.py:7475-7483: remove the extra pixel of a bounding box that does not touch the far edge."""
    (x1, y1, x2, y2), (w, h) = region, image_size
    return x1, y1, x2 - 1 if x2 < w else x2, y2 - 1 if y2 < h else y2


def get_crop_region(bbox, pad, image_size):
    """LD.py:7459-7472 from the mask's bounding box (Image.getbbox: exclusive right / bottom)."""
    (x1, y1, x2, y2), (w, h) = bbox, image_size
    return fix_crop_region((max(x1 - pad, 0), max(y1 - pad, 0), min(x2 + pad, w), min(y2 + pad, h)), image_size)


def expand_crop(region, width, height, target_width, target_height):
    """LD.py:7486-7522: grow the region to the target size, right / bottom first, what does not fit there to the left / top."""
    x1, y1, x2, y2 = region
    x2 = min(x2 + (target_width - (x2 - x1)) // 2, width)
    x1 = max(x1 - (target_width - (x2 - x1)), 0)
    x2 = min(x2 + (target_width - (x2 - x1)), width)
    y2 = min(y2 + (target_height - (y2 - y1)) // 2, height)
    y1 = max(y1 - (target_height - (y2 - y1)), 0)
    y2 = min(y2 + (target_height - (y2 - y1)), height)
    return (x1, y1, x2, y2), (target_width, target_height)


def job_crop(bbox, pad, image_size, tile_size):
    """The crop region process_images takes for a mask with this bounding box (LD.py:7637-7656): padded, then expanded to the tile's
    aspect ratio."""
    x1, y1, x2, y2 = region = get_crop_region(bbox, pad, image_size)
    cw, ch = x2 - x1, y2 - y1
    p_ratio = tile_size[0] / tile_size[1]
    if cw / ch > p_ratio:
        tw, th = cw, round(cw / p_ratio)
    else:
        tw, th = round(ch * p_ratio), ch
    return expand_crop(region, image_size[0], image_size[1], tw, th)[0]


def rectangle_bbox(xi, yi, tile_w, tile_h, image_size):
    """Bounding box of draw.rectangle(calc_rectangle(xi, yi)) (LD.py:7937-7952): inclusive corners, clipped to the image."""
    return xi * tile_w, yi * tile_h, min(xi * tile_w + tile_w + 1, image_size[0]), min(yi * tile_h + tile_h + 1, image_size[1])


def pattern_bbox(pattern: torch.Tensor, px: int, py: int, image_size):
    """Image.getbbox of a black mask with `pattern` [h, w] (host uint8) pasted at (px, py): the non-zero pixels that land on the image."""
    vis = pattern[:max(min(pattern.shape[0], image_size[1] - py), 0), :max(min(pattern.shape[1], image_size[0] - px), 0)] != 0
    rows, cols = vis.any(dim=1).nonzero().flatten(), vis.any(dim=0).nonzero().flatten()
    if rows.numel() == 0:
        raise ValueError("a seam-fix mask has no visible pixel on the canvas")
    return px + int(cols[0]), py + int(rows[0]), px + int(cols[-1]) + 1, py + int(rows[-1]) + 1


def redraw_tile_size(tile_w, tile_h, padding):
    return math.ceil((tile_w + padding) / 8) * 8, math.ceil((tile_h + padding) / 8) * 8


def check_arguments(mode_type, seam_fix_mode, tile_width, tile_height):
    """-> (tile_w, tile_h, redraw enabled, seam fix enabled); ValueError for what the reference would mislabel or the VAE cannot take."""
    if mode_type not in MODES:
        raise ValueError(f"mode_type {mode_type!r}: expected one of {MODES}")
    if seam_fix_mode not in SEAM_FIX_MODES:
        raise ValueError(f"seam_fix_mode {seam_fix_mode!r}: expected one of {SEAM_FIX_MODES}")
    if mode_type == "Chess":
        raise ValueError("mode_type 'Chess' is not supported: the reference runs its LINEAR loop under that name; pass 'Linear'")
    if seam_fix_mode in ("Band Pass", "Half Tile + Intersections"):
        raise ValueError(f"seam_fix_mode {seam_fix_mode!r} is not supported: the reference runs its HALF TILE loop under that name; pass 'Half Tile'")
    tw = tile_width if tile_width > 0 else tile_height
    th = tile_height if tile_height > 0 else tile_width
    if tw <= 0 or th <= 0:
        raise ValueError("tile_width and tile_height cannot both be 0")
    seams = seam_fix_mode == "Half Tile"
    if seams and (tw % 8 or th % 8):
        raise ValueError(f"tile {tw}x{th}: a seam-fix tile is exactly tile_width x tile_height and goes through the VAE, whose stride is 8: "
                         f"both sides must be multiples of 8")
    return tw, th, mode_type == "Linear", seams


def jobs(image_size, tile_w, tile_h, redraw, seams):
    """The reference's job order (LD.py:7945-7958, 8014-8054) as (kind, px, py): 'redraw' rectangles row by row, then the 'row' gradients
    (between vertically adjacent tiles), then the 'col' gradients."""
    rows, cols = math.ceil(image_size[1] / tile_h), math.ceil(image_size[0] / tile_w)
    out = []
    if redraw:
        out += [("redraw", xi * tile_w, yi * tile_h) for yi in range(rows) for xi in range(cols)]
    if seams:
        out += [("row", xi * tile_w, yi * tile_h + tile_h // 2) for yi in range(rows - 1) for xi in range(cols)]
        out += [("col", xi * tile_w + tile_w // 2, yi * tile_h) for yi in range(rows) for xi in range(cols - 1)]
    return out


# ------------------------------------------------------------------ the run
def seam_gradients(ops, tile_w, tile_h, device):
    """row_gradient / col_gradient of half_tile_process (LD.py:7983-8009): Image.linear_gradient("L") (row y holds y) and its rotations,
    BICUBIC-resized to half a tile and pasted into the two halves of a black tile.  -> two uint8 [tile_h, tile_w] on `device`."""
    ramp = torch.arange(256, dtype=torch.uint8)
    down = ramp[:, None].expand(256, 256).contiguous().to(device)          # gradient: value = y
    right = ramp[None, :].expand(256, 256).contiguous().to(device)         # gradient.rotate(90): value = x
    hh, hw = tile_h // 2, tile_w // 2
    row = torch.zeros(tile_h, tile_w, dtype=torch.uint8, device=device)
    col = torch.zeros(tile_h, tile_w, dtype=torch.uint8, device=device)
    if hh > 0:
        row[:hh] = ops.u8_resample(down, (tile_w, hh), "bicubic")
        row[hh:2 * hh] = ops.u8_resample(down.flip(0).contiguous(), (tile_w, hh), "bicubic")         # rotate(180)
    if hw > 0:
        col[:, :hw] = ops.u8_resample(right, (hw, tile_h), "bicubic")
        col[:, hw:2 * hw] = ops.u8_resample(right.flip(1).contiguous(), (hw, tile_h), "bicubic")     # rotate(270)
    return row, col


def default_stages(model, positive, negative, vae, seed, steps, cfg, sampler_name, scheduler, denoise, upscale_model):
    """The product's stages: the resident VAE, sampler and ESRGAN.  Pixels stay on the device; latents go through the host (the posterior
    sample and the sampler's noise are drawn on the host generator, as the reference does)."""
    from . import ops
    from .sampling import common_ksampler
    from .upscale import tiled_upscale
    return SimpleNamespace(
        ops=ops, device=torch.device(model.load_device), observe=None,
        encode=lambda px: {"samples": vae.encode(px)},
        sample=lambda lat: common_ksampler(model, seed, steps, cfg, sampler_name, scheduler, positive, negative, lat, denoise=denoise)[0],
        decode=lambda lat: vae.decode_device(lat["samples"]),
        # ImageUpscaleWithModel.upscale (LD.py:7356-7395); its clamp to [0, 1] is the clip of the quantisation that follows
        upscale_model=lambda img: tiled_upscale(upscale_model, img, 512, 32))


def upscale(image, model, positive, negative, vae, upscale_by, seed, steps, cfg, sampler_name, scheduler, denoise, upscale_model, mode_type,
            tile_width, tile_height, mask_blur, tile_padding, seam_fix_mode, seam_fix_denoise, seam_fix_mask_blur, seam_fix_width,
            seam_fix_padding, force_uniform_tiles, stages=None):
    """UltimateSDUpscale.upscale (LD.py:8236-8324): image [B, H, W, 3] fp32 in [0, 1] -> host fp32 [B, H', W', 3].  See the module
    docstring for the mirrored behaviours.  `stages`: replacement stage callables and op namespace for the orchestration tests (encode,
    sample, decode, upscale_model, ops, device, observe); the product path never passes it."""
    tw, th, redraw, seams = check_arguments(mode_type, seam_fix_mode, tile_width, tile_height)
    st = stages if stages is not None else default_stages(model, positive, negative, vae, seed, steps, cfg, sampler_name, scheduler, denoise,
                                                           upscale_model)
    ops, dev = st.ops, st.device
    if image.dim() != 4 or image.shape[-1] != 3:
        raise ValueError(f"expected an image batch [B, H, W, 3], got {tuple(image.shape)}")
    B, H0, W0, _ = image.shape
    size = W, H = canvas_size(W0, H0, upscale_by)
    factors = get_factors(math.ceil(max(W, H) / max(W0, H0)))

    # tensor_to_pil of every image, the upscale model once per factor on every image, Lanczos to the canvas (LD.py:8276, 7847-7863, 8210-8216)
    batch = list(ops.u8_from_f32(image.to(dev, torch.float32).contiguous()))          # the one upload
    for _ in factors:
        batch = [ops.u8_from_f32(st.upscale_model(ops.f32_from_u8(im)[None]).to(dev, torch.float32))[0] for im in batch]
    canvas = torch.stack([ops.u8_resample(im, size, "lanczos") for im in batch])       # [B, H, W, 3] uint8, resident for the whole run
    row_grad = col_grad = row_host = col_host = None
    if seams:
        row_grad, col_grad = seam_gradients(ops, tw, th, dev)
        row_host, col_host = row_grad.cpu(), col_grad.cpu()                            # tile-sized, once: the bounding boxes are host geometry

    for index, (kind, px, py) in enumerate(jobs(size, tw, th, redraw, seams)):
        if kind == "redraw":
            tile, pad, blur, pattern = redraw_tile_size(tw, th, tile_padding), tile_padding, mask_blur, None
            bbox, rect = rectangle_bbox(px // tw, py // th, tw, th, size), (px, py, tw + 1, th + 1)
        else:
            tile, pad, blur = (tw, th), seam_fix_padding, seam_fix_mask_blur
            pattern = row_grad if kind == "row" else col_grad
            bbox, rect = pattern_bbox(row_host if kind == "row" else col_host, px, py, size), (px, py, tw, th)
        x1, y1, x2, y2 = crop = job_crop(bbox, pad, size, tile)
        alpha = ops.u8_region_mask((H, W), rect, pattern, blur, crop, dev)                             # [y2 - y1, x2 - x1]
        tiles = torch.stack([ops.u8_resample(canvas[b, y1:y2, x1:x2], tile, "lanczos") for b in range(B)])
        latent = st.encode(ops.f32_from_u8(tiles))
        decoded = st.decode(st.sample(latent)).to(dev, torch.float32)
        sampled = ops.u8_from_f32(decoded)
        for b in range(B):
            ops.u8_composite_(canvas[b], ops.u8_resample(sampled[b], (x2 - x1, y2 - y1), "lanczos"), alpha, x1, y1)
        if st.observe is not None:
            st.observe(SimpleNamespace(index=index, kind=kind, crop=crop, tile_size=tile, alpha=alpha, tiles=tiles, canvas=canvas))
    return (ops.f32_from_u8(canvas).cpu(),)                                                            # the one download
