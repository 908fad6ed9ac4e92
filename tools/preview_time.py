"""Timing of the TAESD latent preview -> profiles/preview_time.json.  HIP events (a) / a synchronised wall clock around whole sampler runs
(b), warm-up, median of repeats; everything that is compared runs in ONE process and the variants alternate inside every repeat.
 (a) one TAESD decode of a [1, 4, 64, 64] latent: the captured graph replayed and the eager enqueue, against tests/taesd_ref.py's
     restatement on torch in fp32 (what a reference user gets) and in fp16 channels-last; the per-launch table and FLOP/s over last_flops.
 (b) steps/s of KSampler2 (20 steps, 512 x 512, synthetic SD1.5 weights) at batch 1 and batch 8 with and without a LatentPreviewer on
     image 0 of every step; the overhead in per cent of the same call without the preview.
    python tools/preview_time.py [out.json] [--repeats 7] [--steps 20] [--skip-sampler]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import taesd_ref as TR                             # noqa: E402
from lightdiffusion_amd import nodes as N          # noqa: E402
from lightdiffusion_amd import weights as W        # noqa: E402
from lightdiffusion_amd.preview import LatentPreviewer   # noqa: E402


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "repeats": len(ms)}


def alternate(variants, warmup, repeats, clock):
    """variants: {name: fn}; every repeat runs each once, in order -> {name: [ms]}"""
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in variants}
    for _ in range(repeats):
        for k, fn in variants.items():
            out[k].append(clock(fn))
    return out


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def wall_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "preview_time.json"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--skip-sampler", action="store_true")
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "latent": [1, 4, 64, 64]}
    taesd = N.load_synthetic_taesd("cuda:0")
    sd = {k: W.synth_tensor("taesd_decoder." + k, s).cuda() for k, s in W.taesd_decoder_param_shapes().items()}
    x = torch.randn(1, 4, 64, 64, generator=torch.Generator().manual_seed(0)).cuda()
    with torch.no_grad():
        # ---- (a) the decode alone.  The previewer's own static buffers and graph, without the host copy: _body / _graph.replay
        pv = LatentPreviewer(taesd, lambda i, im: None)
        pv({"x": x, "i": 0, "sigma": 1.0, "denoised": None})
        dec = alternate({"hip_graph_replay": pv._graph.replay, "hip_eager": pv._body,
                         "torch_fp32": lambda: TR.decode(sd, x), "torch_fp16_channels_last": lambda: TR.decode(sd, x, torch.float16, True)},
                        3, a.repeats, event_ms)
        res["decode"] = {k: summary(v) for k, v in dec.items()}
        res["decode"]["previewer_call_with_host_copy"] = summary(
            alternate({"call": lambda: pv({"x": x, "i": 0, "sigma": 1.0, "denoised": None})}, 2, a.repeats, wall_ms)["call"])
        res["launches"], res["total_flops"], res["workspace_bytes"] = taesd.last_launches, taesd.last_flops, taesd.workspace_bytes
        res["decode"]["hip_graph_replay"]["tflops"] = taesd.last_flops / (res["decode"]["hip_graph_replay"]["median_ms"] * 1e-3) * 1e-12
        rows = taesd.profile(x)
        res["launch_table"] = [{"what": w_, "dims": list(d), "flops": fl, "us": us, "kernel": k} for w_, d, fl, us, k in rows]
        per = {}
        for _, _, fl, us, kern in rows:
            k = per.setdefault(kern, {"launches": 0, "ms": 0.0, "flops": 0.0})
            k["launches"] += 1
            k["ms"] += us * 1e-3
            k["flops"] += fl
        for k in per.values():
            k["tflops"] = k["flops"] / (k["ms"] * 1e-3) * 1e-12 if k["ms"] > 0 else 0.0
        res["kernels"] = per

        # ---- (b) the sampler loop with and without the preview
        if not a.skip_sampler:
            model, clip, vae = N.load_synthetic("cuda:0", max_batch=8, max_hw=(64, 64))
            toks = [[(49406, 1.0)] + [(320, 1.0)] * 3 + [(49407, 1.0)] * 73]
            enc = lambda t: clip.encode_from_tokens(t, return_pooled=True)
            (pc, pp), (nc, npool) = enc(toks), enc(toks)
            pos, neg = [[pc, {"pooled_output": pp}]], [[nc, {"pooled_output": npool}]]
            res["sampler"] = {"steps": a.steps, "sampler": "dpmpp_2m_sde", "scheduler": "karras", "size": 512}
            for batch in (1, 8):
                lat = N.EmptyLatentImage().generate(512, 512, batch)[0]
                count = [0]
                pvs = LatentPreviewer(taesd, lambda i, im: count.__setitem__(0, count[0] + 1))
                run = lambda p: N.KSampler2().sample(model, 1, a.steps, 7.0, "dpmpp_2m_sde", "karras", pos, neg, lat, preview=p)
                t = alternate({"without": lambda: run(None), "with": lambda: run(pvs)}, 1, a.repeats, wall_ms)
                wo, wi = statistics.median(t["without"]), statistics.median(t["with"])
                assert count[0] == a.steps * (a.repeats + 1)
                res["sampler"][f"batch{batch}"] = {"without_ms": summary(t["without"]), "with_ms": summary(t["with"]),
                                                   "steps_per_s_without": a.steps / (wo * 1e-3), "steps_per_s_with": a.steps / (wi * 1e-3),
                                                   "overhead_percent": 100.0 * (wi - wo) / wo, "preview_ms_per_step": (wi - wo) / a.steps}
    text = json.dumps(res, indent=1)
    print(text)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
