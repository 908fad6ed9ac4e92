"""What ControlNet costs per step: steps/s through nodes.KSampler2 at 64 x 64 latents (512^2 images), batch 8 and batch 1,
SD1.5-sized synthetic weights, dpmpp_2m_sde / karras, 20 steps, for
  off   the conditioning carries the ControlNet and the keyword is off: the key is inert, the replayed-graph route every existing caller takes
  on    the same conditioning with apply_control=True: the control branch on the [uncond, cond] batch, the UNet pair forward with its residuals
        and the guidance mix, one replayed graph
in ONE process on one box, every shape warmed up first, the two variants alternating run by run.  A run is timed with a host clock around
KSampler2().sample between two device synchronises (the call ends with the samples on the host); the figure per variant is the median over the
runs, with the minimum and the maximum beside it.  Beside them:
  hint_encoder_ms       the eight launches of MI355XControlNet.set_hint for a 512 x 512 image: HIP events around back-to-back calls, per call
  flops                 ld_unet_last_flops of both handles for one guided step (algorithmic work of the 2B-sample forwards) and the control
                        branch's share of their sum
  time_ratio, flop_ratio   on / off step time against (UNet + control) / UNet FLOPs: how far the control branch's time is from its share of the work
Nothing is gated here; the numbers are the record.

    python tools/control_cost.py [--steps 20] [--repeats 5] [--batches 8 1] [--out profiles/control_cost.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = W = 64
SAMPLER, SCHEDULER, CFG = "dpmpp_2m_sde", "karras", 7.0


def toks(word):
    return [[(49406, 1.0)] + [(word, 1.0)] * 3 + [(49407, 1.0)] * 73]


def summary(xs, steps):
    med = statistics.median(xs)
    return {"median_ms_per_step": med, "min_ms_per_step": min(xs), "max_ms_per_step": max(xs), "steps_per_s": 1e3 / med, "runs": len(xs), "steps": steps}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 1])
    ap.add_argument("--tiny", action="store_true", help="the tiny configuration (a rehearsal of the tool, not a measurement)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "control_cost.json"))
    a = ap.parse_args(argv)
    sys.path.insert(0, ROOT)
    import torch
    from lightdiffusion_amd import nodes as N
    if not torch.cuda.is_available():
        raise SystemExit("control_cost.py measures on the GPU; none is visible")
    dev = "cuda:0"
    model, clip, _ = N.load_synthetic(dev, max_batch=max(a.batches), max_hw=(H, W), tiny=a.tiny)
    cn = N.load_synthetic_controlnet(dev, max_batch=max(a.batches), max_hw=(H, W), tiny=a.tiny)
    unet = model.model_options["model_function_wrapper"]
    enc = lambda t: [[c, {"pooled_output": p}] for c, p in [clip.encode_from_tokens(t, return_pooled=True)]]
    pos, neg = enc(toks(320)), enc(toks(2368))
    image = torch.rand(1, 8 * H, 8 * W, 3, generator=torch.Generator().manual_seed(1))
    cpos = N.ControlNetApply().apply_controlnet(pos, cn, image, 1.0)[0]

    def one(b, on):
        lat = {"samples": torch.zeros(b, 4, H, W)}
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = N.KSampler2().sample(model, 0, a.steps, CFG, SAMPLER, SCHEDULER, cpos, neg, lat, apply_control=on)[0]["samples"]
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t) * 1e3 / a.steps
        assert torch.isfinite(out).all()
        return ms

    res = {"what": f"ControlNet through nodes.KSampler2, {H} x {W} latents, {'tiny' if a.tiny else 'SD1.5-sized'} synthetic weights, {SAMPLER} / "
                   f"{SCHEDULER}, cfg {CFG}, {a.steps} steps a run, strength 1, one 512 x 512 hint",
           "how": "one process; every shape warmed up, off / on alternating run by run; a run = host clock around KSampler2().sample between device "
                  "synchronises, over its steps; hint encoder = HIP events around back-to-back set_hint calls; flops = ld_unet_last_flops of the UNet "
                  "handle and of the control handle after a controlled step", "batches": {}}
    for b in a.batches:
        for on in (False, True):                                  # warm-up: code objects, workspaces, both captured graphs of the shape
            one(b, on)
        runs = {False: [], True: []}
        for _ in range(a.repeats):
            for on in (False, True):
                runs[on].append(one(b, on))
        off, on = summary(runs[False], a.steps), summary(runs[True], a.steps)
        unet_flops, ctl_flops = unet.last_flops, cn.control_model.last_flops      # the last step of the last (controlled) run: 2b samples each
        row = {"off": off, "on": on, "unet_flops_per_step": unet_flops, "control_flops_per_step": ctl_flops,
               "control_share_of_flops": ctl_flops / (unet_flops + ctl_flops),
               "flop_ratio": (unet_flops + ctl_flops) / unet_flops, "time_ratio": on["median_ms_per_step"] / off["median_ms_per_step"]}
        res["batches"][str(b)] = row
    # the hint encoder on its own: a 512 x 512 image, hint batch 1
    cm = cn.control_model
    hint = image.movedim(-1, 1).to(dev).contiguous()
    for _ in range(3):
        cm.set_hint(hint)
    n = 20
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(n):
        cm.set_hint(hint)
    e.record()
    torch.cuda.synchronize()
    flops = 0.0
    chain = (3,) + tuple(cm.param_shapes()[f"input_hint_block.{2 * i}.weight"][0] for i in range(8))
    side = 8 * H
    for i in range(8):
        stride = 2 if i in (2, 4, 6) else 1
        side = side // stride
        flops += 2.0 * side * side * chain[i + 1] * 9 * chain[i]
    ms = s.elapsed_time(e) / n
    res["hint_encoder"] = {"image": f"{8 * H} x {8 * W}", "ms": ms, "gflop": flops * 1e-9, "tflops": flops / ms * 1e-9, "launches": 8}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
