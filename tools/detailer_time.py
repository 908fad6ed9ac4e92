"""Times ONE Detailer pass on the device at the reference's settings (its pipeline's DetailerForEach calls, LD.py:10646-10725): a 512^2 image, one
segment with a 256^2 crop, guide_size 512, max_size 768 (so the crop is redrawn at 512^2: 64 x 64 latents), 40 steps dpmpp_2m_sde / karras,
denoise 0.5, cfg 6.5, feather 5, on SD1.5-sized synthetic weights.  Per segment: each of the six image ops detailer.do_detail issues (HIP events
around every call, summed per op) and the encode / sample / decode stages (a host clock around work that ends in a device synchronise: they
move latents through the host).  One untimed warm-up pass, then the median of the repeats.

    python tools/detailer_time.py [--repeats 3] [--out profiles/detailer_time.json]
"""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lightdiffusion_amd import detailer as D   # noqa: E402
from lightdiffusion_amd import nodes as N      # noqa: E402
from lightdiffusion_amd import ops             # noqa: E402

IMAGE, BOX = 512, (192.0, 192.0, 320.0, 320.0)          # crop_factor 2 about a 128^2 box: the crop is [128, 128, 384, 384]
SETTINGS = dict(guide_size=512, max_size=768, steps=40, cfg=6.5, sampler_name="dpmpp_2m_sde", scheduler="karras", denoise=0.5, feather=5)
OPS = ("f32_gaussian_blur", "u8_crop_from_f32", "u8_resample", "f32_from_u8", "u8_from_f32", "f32_paste_u8_")
STAGES = ("encode", "sample", "decode")


def timed_ops(log):
    """The op namespace with HIP events around every call of the six ops -> log: [(name, start, end)]."""
    def wrap(name):
        f = getattr(ops, name)

        def call(*a, **kw):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            out = f(*a, **kw)
            e.record()
            log.append((name, s, e))
            return out
        return call
    return SimpleNamespace(**{name: wrap(name) for name in OPS})


def timed_stage(f, name, log):
    def call(*a):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = f(*a)
        torch.cuda.synchronize()
        log.append((name, (time.perf_counter() - t) * 1e3))
        return out
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "detailer_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("detailer_time.py measures on the GPU; none is visible")
    model, clip, vae = N.load_synthetic("cuda:0", max_batch=1, max_hw=(64, 64))
    toks = [[(49406, 1.0)] + [(320, 1.0)] * 3 + [(49407, 1.0)] * 73]
    c, p = clip.encode_from_tokens(toks, return_pooled=True)
    cond = [[c, {"pooled_output": p}]]
    image = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (1, IMAGE, IMAGE, 3), dtype=np.uint8).astype(np.float32) / np.float32(255.0))
    segs = D.segs_from_boxes(image, [BOX], crop_factor=2.0)
    assert list(segs[1][0].crop_region) == [128, 128, 384, 384]
    s = SETTINGS
    assert D.work_size(256, 256, s["guide_size"], s["max_size"]) == (512, 512, 512, 512)

    def one_pass():
        op_log, stage_log = [], []
        st = D.model_stages(model, vae, cond, cond, s["steps"], s["cfg"], s["sampler_name"], s["scheduler"], s["denoise"], ops=timed_ops(op_log))
        for name in STAGES:
            setattr(st, name, timed_stage(getattr(st, name), name, stage_log))
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = D.do_detail(image, segs, model, clip, vae, s["guide_size"], True, s["max_size"], 0, s["steps"], s["cfg"], s["sampler_name"], s["scheduler"],
                          cond, cond, s["denoise"], s["feather"], True, True, "", stages=st)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t) * 1e3
        assert torch.isfinite(out[0]).all() and len(out[1]) == 1
        per_op = {name: 0.0 for name in OPS}
        calls = {name: 0 for name in OPS}
        for name, start, end in op_log:
            per_op[name] += start.elapsed_time(end)
            calls[name] += 1
        per_stage = {name: sum(ms for n, ms in stage_log if n == name) for name in STAGES}
        return per_op, calls, per_stage, wall

    one_pass()                                    # warm-up: code objects, workspaces, tap and coefficient uploads
    runs = [one_pass() for _ in range(a.repeats)]
    med = lambda xs: statistics.median(xs)
    image_ops = {name: {"median_ms": med([r[0][name] for r in runs]), "calls": runs[0][1][name]} for name in OPS}
    stages = {name: {"median_ms": med([r[2][name] for r in runs])} for name in STAGES}
    ops_ms, stages_ms, wall_ms = med([sum(r[0].values()) for r in runs]), med([sum(r[2].values()) for r in runs]), med([r[3] for r in runs])
    res = {"what": "one Detailer segment: 512^2 image, 256^2 crop redrawn at 512^2, SD1.5-sized synthetic weights", "settings": s, "repeats": a.repeats,
           "image_ops": image_ops, "image_ops_total_ms": ops_ms, "stages": stages, "stages_total_ms": stages_ms, "pass_wall_ms": wall_ms,
           "image_ops_share_of_pass": ops_ms / wall_ms,
           "how": "image ops: HIP events around each call, summed per op; stages and the pass: host clock around a device synchronise"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
