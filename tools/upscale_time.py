"""Timing of the ESRGAN upscaler: the full x4 nb-23 model on one 512 x 512 tile and the ImageUpscaleWithModel node on one 512 x 512 image
(four tiles), against tests/esrgan_ref.py's restatement on torch in fp32 (what a reference user gets) and in fp16 channels-last (the obvious
alternative), same process, same order.  Warm-up, HIP events, median of repeats -> profiles/upscale_time.json.
    python tools/upscale_time.py [out.json] [--size 512] [--repeats 5]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import esrgan_ref as ER                           # noqa: E402
from lightdiffusion_amd import nodes as N         # noqa: E402
from lightdiffusion_amd import weights as W       # noqa: E402

PEAK_FP16_DENSE = 2.5e15      # MI355X dense fp16 matrix rate (MI355X_MICROARCH.md), FLOP/s


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "repeats": repeats}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "upscale_time.json"))
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--nb", type=int, default=23)
    a = ap.parse_args()
    nb, scale, S = a.nb, 4, a.size
    m = N.load_synthetic_upscaler("cuda:0", nb=nb, scale=scale)
    sd = {k: v.cuda() for k, v in W.synth_state_dict(W.esrgan_param_shapes(W.esrgan_config(nb, scale))).items()}
    x = torch.rand(1, S, S, 3, generator=torch.Generator().manual_seed(0)).cuda()
    res = {"size": S, "nb": nb, "scale": scale, "device": torch.cuda.get_device_name(0)}
    with torch.no_grad():
        res["hip_model_tile"] = timed(lambda: m.forward_device(x), 2, a.repeats)
        res["workspace_bytes"] = m.workspace_bytes
        node = N.ImageUpscaleWithModel()
        res["hip_node_image"] = timed(lambda: node.upscale(m, x), 1, max(3, a.repeats // 2))
        res["torch_fp32"] = timed(lambda: ER.rrdbnet(sd, x, nb, scale, torch.float32), 1, 3)
        res["torch_fp16_channels_last"] = timed(lambda: ER.rrdbnet(sd, x, nb, scale, torch.float16, channels_last=True), 1, 3)
    rows = m.profile(x)
    per = {}
    for what, dims, fl, us, kern in rows:
        k = per.setdefault(kern, {"launches": 0, "ms": 0.0, "flops": 0.0})
        k["launches"] += 1
        k["ms"] += us * 1e-3
        k["flops"] += fl
    for k in per.values():
        k["tflops"] = k["flops"] / (k["ms"] * 1e-3) * 1e-12 if k["ms"] > 0 else 0.0
    res["kernels"] = per
    trunk = [r for r in rows if r[0] == "dense3" and r[1][0] == S * S and (r[1][1] == 32 or r[1][2] == 9 * 192)]
    t_ms, t_fl = sum(r[3] for r in trunk) * 1e-3, sum(r[2] for r in trunk)
    res["trunk"] = {"launches": len(trunk), "ms": t_ms, "flops": t_fl, "tflops": t_fl / (t_ms * 1e-3) * 1e-12,
                    "share_of_fp16_dense_peak": t_fl / (t_ms * 1e-3) / PEAK_FP16_DENSE}
    res["total_flops"] = m.last_flops
    text = json.dumps(res, indent=1)
    print(text)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
