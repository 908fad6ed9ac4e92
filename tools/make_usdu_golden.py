"""Writes the UltimateSDUpscale fixtures of tests/golden/ from the reference's own node and from Pillow.

The reference is read where it lies (LD_REFERENCE, as oracle/extract_ref.py does): the file is parsed and a whitelist of the top-level
nodes between `flatten` and the end of `UltimateSDUpscale` is executed in source order — definitions, plain assignments and the module-level
monkey patches (`USDUpscaler.__init__ = new_init` and the like); none of its text is copied.  The four expensive stages are replaced by
deterministic closed-form stand-ins (below, restated in tests/usdu_standins.py), exact in fp32 whatever the order of evaluation, so the
fixtures pin the node's geometry, masks and PIL plumbing and nothing else.

  tests/golden/usdu_flow.npz  per record (B = 1, B = 2): input, parameters and, for every process_images call, the crop region, the tile
                              size, the blurred mask inside the region, the tiles handed to the encoder and the canvas inside the region
                              after the composite (outside it process_images leaves the canvas alone); the final image
  tests/golden/usdu_ops.npz   Pillow's own outputs for the three ops on the small cases of tests/test_usdu_gpu.py

    python tools/make_usdu_golden.py
"""
import ast
import math
import os
import sys
from enum import Enum

import numpy as np
import torch
from PIL import Image, ImageDraw, ImageFilter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import usdu_standins as S                      # noqa: E402
from oracle.extract_ref import REF_PATH        # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
NAMES = {"torch_gc", "flatten", "Script", "Options", "State", "opts", "state", "sd_upscalers", "actual_upscaler", "batch", "tensor_to_pil",
         "pil_to_tensor", "get_crop_region", "fix_crop_region", "expand_crop", "crop_cond", "Upscaler", "UpscalerData", "StableDiffusionProcessing",
         "Processed", "fix_seed", "process_images", "USDUMode", "USDUSFMode", "USDUpscaler", "USDURedraw", "USDUSeamsFix", "old_init", "new_init",
         "old_setup_redraw", "new_setup_redraw", "old_setup_seams_fix", "new_setup_seams_fix", "old_upscale", "new_upscale", "MODES",
         "SEAM_FIX_MODES", "UltimateSDUpscale"}
PATCHED = {("USDUpscaler", "__init__"), ("USDURedraw", "init_draw"), ("USDUSeamsFix", "init_draw"), ("USDUpscaler", "upscale")}


def load_reference():
    ns = {"torch": torch, "np": np, "math": math, "Enum": Enum, "Image": Image, "ImageDraw": ImageDraw, "ImageFilter": ImageFilter,
          "__name__": "ld_reference_usdu"}
    body = ast.parse(open(REF_PATH).read(), REF_PATH).body
    first = next(n.lineno for n in body if getattr(n, "name", None) == "torch_gc")
    last = next(n.end_lineno for n in body if getattr(n, "name", None) == "UltimateSDUpscale")
    found = set()
    for node in body:
        if not first <= node.lineno <= last:
            continue
        name = getattr(node, "name", None)
        if name is None and isinstance(node, ast.Assign):
            t = node.targets[0]
            if isinstance(t, ast.Name):
                name = t.id
            elif isinstance(t, ast.Attribute) and isinstance(t.value, ast.Name) and (t.value.id, t.attr) in PATCHED:
                name = (t.value.id, t.attr)
        if name in NAMES or name in PATCHED:
            exec(compile(ast.Module([node], []), REF_PATH, "exec"), ns)
            found.add(name)
    missing = (NAMES | PATCHED) - found
    if missing:
        raise RuntimeError(f"reference nodes not found: {sorted(map(str, missing))}")
    return ns


def run_flow(ns, image, params):
    """One UltimateSDUpscale.upscale of the reference with the stand-in stages, recording every process_images call."""
    rec = {"crop": [], "tile_size": [], "alpha": [], "tiles": [], "after": []}

    class VAEEncode:
        def encode(self, vae, pixels):
            rec["tiles"].append(S.as_u8(pixels))
            return (S.encode(pixels),)

    class VAEDecode:
        def decode(self, vae, samples):
            return (S.decode(samples),)

    class ImageUpscaleWithModel:
        def upscale(self, upscale_model, image):
            return (S.upscale_model(image),)

    def common_ksampler(model, seed, steps, cfg, sampler_name, scheduler, positive, negative, latent, denoise=1.0):
        return (S.sample(latent),)

    expand_crop, process_images = ns["expand_crop"], ns["process_images"]

    def recording_expand_crop(*a):
        out = expand_crop(*a)
        rec["crop"].append(out[0])
        return out

    def recording_process_images(p):
        mask = p.image_mask.convert("L")
        blur = p.mask_blur
        out = process_images(p)
        crop = rec["crop"][-1]
        rec["tile_size"].append((p.width, p.height))
        rec["alpha"].append(np.array((mask.filter(ImageFilter.GaussianBlur(blur)) if blur > 0 else mask).crop(crop)))
        rec["after"].append(np.stack([np.array(im.crop(crop)) for im in ns["batch"]]))
        return out

    ns.update(VAEEncode=VAEEncode, VAEDecode=VAEDecode, ImageUpscaleWithModel=ImageUpscaleWithModel, common_ksampler=common_ksampler,
              expand_crop=recording_expand_crop, process_images=recording_process_images)
    (final,) = ns["UltimateSDUpscale"]().upscale(image=image, model=None, positive=[], negative=[], vae=None, upscale_model=None, seed=1, steps=2,
                                                 cfg=1.0, sampler_name="euler", scheduler="normal", force_uniform_tiles="enable", **params)
    ns.update(expand_crop=expand_crop, process_images=process_images)
    return rec, S.as_u8(final)


def flow_fixture(ns):
    out = {}
    params = dict(S.FLOW_PARAMS)
    for k, v in params.items():
        out["param_" + k] = np.array(v)
    for tag, b in (("b1", 1), ("b2", 2)):
        image = S.flow_input(b)
        rec, final = run_flow(ns, image, params)
        out[f"{tag}_input"] = S.as_u8(image)
        out[f"{tag}_crop"] = np.array(rec["crop"], np.int32)
        out[f"{tag}_tile_size"] = np.array(rec["tile_size"], np.int32)
        out[f"{tag}_final"] = final
        for j in range(len(rec["crop"])):
            out[f"{tag}_alpha_{j:02d}"] = rec["alpha"][j]
            out[f"{tag}_tiles_{j:02d}"] = rec["tiles"][j]
            out[f"{tag}_after_{j:02d}"] = rec["after"][j]
        print(tag, "jobs", len(rec["crop"]), "final", final.shape)
    np.savez_compressed(os.path.join(GOLDEN, "usdu_flow.npz"), **out)


def ops_fixture():
    out = {}
    for name, (src, box, size, filt) in S.resample_cases().items():
        im = Image.fromarray(src)
        if box is not None:
            im = im.crop(box)
        out["resample_" + name] = np.array(im.resize(size, {"lanczos": Image.LANCZOS, "bicubic": Image.BICUBIC}[filt]))
    for name, (mask, radius) in S.blur_cases().items():
        out["blur_" + name] = np.array(Image.fromarray(mask).filter(ImageFilter.GaussianBlur(radius)))
    for name, (canvas, tile, alpha, x0, y0) in S.composite_cases().items():
        # the chain of process_images (paste, double putalpha, masked paste, alpha_composite, convert) on Pillow itself
        init = Image.fromarray(canvas)
        tile_only = Image.new("RGBA", init.size)
        tile_only.paste(Image.fromarray(tile), (x0, y0))
        mask = np.zeros(canvas.shape[:2], np.uint8)
        mask[y0:y0 + alpha.shape[0], x0:x0 + alpha.shape[1]] = alpha
        temp = tile_only.copy()
        temp.putalpha(Image.fromarray(mask))
        temp.putalpha(Image.fromarray(mask))
        tile_only.paste(temp, tile_only)
        result = init.convert("RGBA")
        result.alpha_composite(tile_only)
        out["composite_" + name] = np.array(result.convert("RGB"))
    np.savez_compressed(os.path.join(GOLDEN, "usdu_ops.npz"), **out)


if __name__ == "__main__":
    ops_fixture()
    flow_fixture(load_reference())
    for f in ("usdu_ops.npz", "usdu_flow.npz"):
        print(f, os.path.getsize(os.path.join(GOLDEN, f)), "bytes")
