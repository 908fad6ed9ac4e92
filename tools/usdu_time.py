"""Times the image plumbing of ONE UltimateSDUpscale tile job on the device, at the reference's sizes: a 1024^2 canvas, a 576^2 crop
resampled to a 544^2 tile and back, mask blur 16.  The chain is the one usdu.upscale issues per job: region mask + blur, crop-resample
in, /255, (stages), quantise, resample out, composite.  HIP events around the whole chain, warm-up first, the median of the repeats.
Next to it: the same chain with Pillow on this host (where Pillow imports; otherwise tests/usdu_ref.py, labelled as such), and, for scale,
the encode, sampler and decode of the same job on SD1.5-sized synthetic weights.

    python tools/usdu_time.py [--repeats 50] [--out profiles/usdu_time.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from lightdiffusion_amd import nodes as N      # noqa: E402
from lightdiffusion_amd import ops             # noqa: E402

CANVAS, CROP, TILE, BLUR = 1024, (224, 224, 800, 800), 544, 16
RECT = (256, 256, 513, 513)


def device_chain(canvas, decoded):
    x1, y1, x2, y2 = CROP
    alpha = ops.u8_region_mask((CANVAS, CANVAS), RECT, None, BLUR, CROP, canvas.device)
    px = ops.f32_from_u8(ops.u8_resample(canvas[y1:y2, x1:x2], (TILE, TILE), "lanczos"))
    back = ops.u8_resample(ops.u8_from_f32(decoded), (x2 - x1, y2 - y1), "lanczos")
    ops.u8_composite_(canvas, back, alpha, x1, y1)
    return px


def events_ms(fn, repeats, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times), "repeats": repeats}


def host_chain(canvas, decoded):
    """process_images' plumbing (LD.py:7659-7736) on the host -> (label, callable)."""
    x1, y1, x2, y2 = CROP
    try:
        from PIL import Image, ImageDraw, ImageFilter
    except ImportError:
        import usdu_ref as R

        def ref():
            mask = np.zeros((CANVAS, CANVAS), np.uint8)
            mask[RECT[1]:RECT[1] + RECT[3], RECT[0]:RECT[0] + RECT[2]] = 255
            alpha = R.gaussian_blur(mask, BLUR)[y1:y2, x1:x2]
            R.to_f32(R.resample(canvas[y1:y2, x1:x2], TILE, TILE))
            R.composite(canvas, R.resample(R.to_u8(decoded), x2 - x1, y2 - y1), alpha, x1, y1)
        return "tests/usdu_ref.py (NumPy; Pillow does not import here)", ref

    def pil():
        init = Image.fromarray(canvas)
        mask = Image.new("L", init.size, "black")
        ImageDraw.Draw(mask).rectangle((RECT[0], RECT[1], RECT[0] + RECT[2] - 1, RECT[1] + RECT[3] - 1), fill="white")
        mask = mask.filter(ImageFilter.GaussianBlur(BLUR))
        tile = init.crop(CROP).resize((TILE, TILE), Image.LANCZOS)
        np.array(tile).astype(np.float32) / 255.0
        sampled = Image.fromarray(np.clip(255.0 * decoded, 0, 255).astype(np.uint8)).resize((x2 - x1, y2 - y1), Image.LANCZOS)
        only = Image.new("RGBA", init.size)
        only.paste(sampled, CROP[:2])
        temp = only.copy()
        temp.putalpha(mask)
        temp.putalpha(mask)
        only.paste(temp, only)
        result = init.convert("RGBA")
        result.alpha_composite(only)
        result.convert("RGB")
    return "Pillow " + __import__("PIL").__version__, pil


def host_ms(fn, repeats):
    fn()
    times = []
    for _ in range(repeats):
        t = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t) * 1e3)
    return {"median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times), "repeats": repeats}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "usdu_time.json"))
    ap.add_argument("--no-stages", action="store_true", help="skip the encode / sampler / decode timing")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("usdu_time.py measures on the GPU; none is visible")
    rng = np.random.default_rng(0)
    canvas_h = rng.integers(0, 256, (CANVAS, CANVAS, 3), dtype=np.uint8)
    decoded_h = rng.random((TILE, TILE, 3), dtype=np.float32)
    canvas, decoded = torch.from_numpy(canvas_h).cuda(), torch.from_numpy(decoded_h).cuda()
    res = {"canvas": CANVAS, "crop": CROP[2] - CROP[0], "tile": TILE, "mask_blur": BLUR,
           "device_plumbing": events_ms(lambda: device_chain(canvas, decoded), a.repeats)}
    label, fn = host_chain(canvas_h.copy(), decoded_h)
    res["host_plumbing"] = dict(host_ms(fn, max(5, a.repeats // 5)), what=label)
    if not a.no_stages:
        model, clip, vae = N.load_synthetic("cuda:0", max_batch=1, max_hw=(68, 68))
        toks = [[(49406, 1.0)] + [(320, 1.0)] * 3 + [(49407, 1.0)] * 73]
        c, p = clip.encode_from_tokens(toks, return_pooled=True)
        cond = [[c, {"pooled_output": p}]]
        px = device_chain(canvas, decoded)[None]
        lat = {"samples": vae.encode(px)}
        sample = lambda: N.KSampler2().sample(model, 1, 8, 6, "euler_ancestral", "karras", cond, cond, lat, denoise=0.3)[0]
        out = sample()
        wall = lambda f: host_ms(lambda: (f(), torch.cuda.synchronize()), 10)
        res["stages"] = {"what": "SD1.5-sized synthetic weights, 544^2 tile (68 x 68 latents), wall clock around a synchronise",
                         "vae_encode": wall(lambda: vae.encode(px)), "sampler_8_steps_denoise_0.3": wall(sample),
                         "vae_decode": wall(lambda: vae.decode_device(out["samples"]))}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
