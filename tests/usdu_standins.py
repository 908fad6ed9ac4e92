"""Shared by tools/make_usdu_golden.py and the UltimateSDUpscale tests: the closed-form stand-in stages the flow fixture was recorded
with, the inputs of the op cases, and `RefOps`, the NumPy restatement (usdu_ref) behind the op seam of lightdiffusion_amd.usdu.

The stand-ins are exact in fp32 whatever the order of evaluation (max / min pooling, single products and sums), so they give the same
bytes on every machine and on the device."""
from types import SimpleNamespace

import numpy as np
import torch

import usdu_ref as R

# 40 x 48 input (W x H), upscale_by 2 -> an 80 x 96 canvas, tile 32 -> a 3 x 3 grid: 9 redraw jobs and 12 seam jobs
FLOW_PARAMS = dict(upscale_by=2, denoise=0.3, mode_type="Linear", tile_width=32, tile_height=32, mask_blur=4, tile_padding=8,
                   seam_fix_mode="Half Tile", seam_fix_denoise=0.2, seam_fix_mask_blur=4, seam_fix_width=16, seam_fix_padding=8)
FLOW_JOBS = 21


def flow_params():
    return dict(FLOW_PARAMS)


def flow_input(b):
    """[b, 48, 40, 3] fp32 in [0, 1], values k / 255."""
    rng = np.random.default_rng(20 + b)
    return torch.from_numpy(R.to_f32(rng.integers(0, 256, (b, 48, 40, 3), dtype=np.uint8)))


def as_u8(x):
    """uint8 of an fp32 tensor that holds k / 255 values."""
    return (x.detach().cpu().float() * 255.0).round().clamp(0, 255).to(torch.uint8).numpy()


# ---- the stand-in stages
def encode(pixels):
    """[B, h, w, 3] -> {"samples": [B, 4, h / 8, w / 8]}: 8 x 8 max pool of r, g, b and the min pool of g."""
    p = pixels.detach().cpu().float().movedim(-1, 1)
    b, c, h, w = p.shape
    blocks = p.reshape(b, c, h // 8, 8, w // 8, 8)
    return {"samples": torch.cat([blocks.amax(dim=(3, 5)), blocks[:, 1:2].amin(dim=(3, 5))], dim=1)}


def sample(latent):
    """adds a fixed pattern"""
    s = latent["samples"]
    c, y, x = torch.meshgrid(torch.arange(s.shape[1]), torch.arange(s.shape[2]), torch.arange(s.shape[3]), indexing="ij")
    return {"samples": s + (((c + 2 * y + 3 * x) % 5 - 2).float() * 0.0625)[None]}


def decode(latent):
    """nearest x 8 with a colour affine (values leave [0, 1]: the quantisation's clip is exercised)"""
    s = latent["samples"].detach().cpu().float()
    rgb = s[:, :3] * 0.75 + s[:, 3:4] * 0.25
    return rgb.repeat_interleave(8, dim=2).repeat_interleave(8, dim=3).movedim(1, -1).contiguous()


def upscale_model(image):
    """nearest x 4 of [B, H, W, 3]"""
    return image.detach().cpu().float().repeat_interleave(4, dim=1).repeat_interleave(4, dim=2).contiguous()


# ---- the op seam on the NumPy restatement
class RefOps:
    """lightdiffusion_amd.ops' five uint8 image ops on host tensors, computed by usdu_ref."""

    @staticmethod
    def u8_from_f32(x):
        return torch.from_numpy(R.to_u8(x.numpy()))

    @staticmethod
    def f32_from_u8(x):
        return torch.from_numpy(R.to_f32(x.numpy()))

    @staticmethod
    def u8_resample(src, size, filt="lanczos"):
        return torch.from_numpy(R.resample(src.numpy(), size[0], size[1], filt))

    @staticmethod
    def u8_region_mask(hw, rect, pattern, radius, region, device):
        mask = np.zeros(hw, np.uint8)
        x, y, w, h = rect
        h, w = min(h, hw[0] - y), min(w, hw[1] - x)
        mask[y:y + h, x:x + w] = 255 if pattern is None else pattern.numpy()[:h, :w]
        if radius > 0:
            mask = R.gaussian_blur(mask, radius)
        return torch.from_numpy(np.ascontiguousarray(mask[region[1]:region[3], region[0]:region[2]]))

    @staticmethod
    def u8_composite_(canvas, tile, alpha, x0, y0):
        R.composite(canvas.numpy(), tile.numpy(), alpha.numpy(), x0, y0)      # in place: the tensor shares the array
        return canvas


def standin_stages(ops, device, observe=None):
    return SimpleNamespace(ops=ops, device=torch.device(device), observe=observe, encode=encode, sample=sample, decode=decode,
                           upscale_model=upscale_model)


# ---- op cases (inputs from seeds; Pillow's outputs are in tests/golden/usdu_ops.npz)
def _rand(seed, shape):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def resample_cases():
    """name -> (source image, crop box (x1, y1, x2, y2) or None, (out_w, out_h), filter)"""
    big = _rand(1, (96, 80, 3))
    grad = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 256, axis=1)
    return {
        "mixed": (_rand(0, (37, 53, 3)), None, (72, 24), "lanczos"),            # height down, width up, ragged widths
        "window_in": (big, (21, 30, 68, 78), (40, 40), "lanczos"),               # a 47 x 48 window at a nonzero origin
        "window_out": (_rand(2, (40, 40, 3)), None, (47, 48), "lanczos"),        # and back
        "identity_h": (_rand(3, (30, 30, 3)), None, (17, 30), "lanczos"),        # the vertical pass is skipped
        "identity_w": (_rand(4, (30, 30, 3)), None, (30, 41), "lanczos"),        # the horizontal pass is skipped
        "one_row": (_rand(5, (1, 9, 3)), None, (20, 1), "lanczos"),
        "gradient": (grad, None, (32, 16), "bicubic"),                           # one channel: the seam-fix gradient
    }


def blur_cases():
    """name -> (mask, radius)"""
    rect = np.zeros((96, 80), np.uint8)
    rect[0:41, 39:80] = 255                                                      # touches the top and the right edge
    return {"rect_r4": (rect, 4), "r16": (_rand(6, (96, 120)), 16), "r2p5": (_rand(7, (50, 70)), 2.5)}


def composite_cases():
    """name -> (canvas, tile, alpha, x0, y0)"""
    alpha = _rand(10, (10, 13))
    alpha[0], alpha[1] = 0, 255
    return {"inner": (_rand(8, (30, 41, 3)), _rand(9, (10, 13, 3)), alpha, 5, 7),
            "corner": (_rand(11, (30, 41, 3)), _rand(12, (10, 13, 3)), _rand(13, (10, 13)), 28, 20)}     # flush with the far corner
