"""What the masked sampler route costs per step: ms per sampler step through nodes.KSampler2 at 64 x 64 latents (512^2 images),
batch 1 and batch 8, SD1.5-sized synthetic weights, dpmpp_2m_sde / karras, for
  unmasked    no mask, no option: the route every existing caller takes
  masked      SetLatentNoiseMask + apply_noise_mask=True: the two blend launches around every model call
  masked_dd   the same on a model that carries DifferentialDiffusion's denoise-mask function (its per-step threshold and comparison on the device)
and, with --parent-tree DIR (a checkout of the parent commit with its library built), the parent's unmasked step on the same box in the same
session.  Every tree is measured in a fresh child process of its own, one at a time, the trees alternating (--rounds); inside a process every
shape is warmed up first and the variants alternate run by run.  A run is timed with a host clock around KSampler2().sample between two device
synchronises (the call ends with the samples on the host) and divided by its steps; the figure per variant is the median over all runs, with the
minimum and maximum beside it.  The two blend kernels are also timed on their own: HIP events around a few hundred back-to-back in / out pairs
on latents of the batch's size, per pair — the kernels' time plus their launch gaps, which is what the masked route should add to a step.

    python tools/inpaint_cost.py [--parent-tree DIR] [--steps 30] [--repeats 5] [--rounds 2] [--out profiles/inpaint_cost.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOKS = [[(49406, 1.0)] + [(320, 1.0)] * 3 + [(49407, 1.0)] * 73]
NEG = [[(49406, 1.0)] + [(49407, 1.0)] * 76]
H = W = 64
SAMPLER, SCHEDULER, CFG = "dpmpp_2m_sde", "karras", 7.0


def child(a):
    """One tree, one process: {batch: {variant: [ms per step, ...]}} (and the blend pair's time) as one JSON line on stdout."""
    sys.path.insert(0, os.path.abspath(a.package_root))
    import torch
    from lightdiffusion_amd import nodes as N
    from lightdiffusion_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("inpaint_cost.py measures on the GPU; none is visible")
    variants = a.variants.split(",")
    model, clip, _ = N.load_synthetic("cuda:0", max_batch=max(a.batches), max_hw=(H, W))
    enc = lambda t: [[c, {"pooled_output": p}] for c, p in [clip.encode_from_tokens(t, return_pooled=True)]]
    pos, neg = enc(TOKS), enc(NEG)
    mask = torch.ones(8 * H, 8 * W)
    mask[:, : 4 * W] = 0.0
    models = {"unmasked": model, "masked": model}
    if "masked_dd" in variants:
        models["masked_dd"] = N.DifferentialDiffusion().apply(model)[0]

    def one(b, variant):
        lat = {"samples": torch.zeros(b, 4, H, W)}
        kw = {}
        if variant != "unmasked":
            lat = N.SetLatentNoiseMask().set_mask(lat, mask)[0]
            kw["apply_noise_mask"] = True
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = N.KSampler2().sample(models[variant], 0, a.steps, CFG, SAMPLER, SCHEDULER, pos, neg, lat, **kw)[0]["samples"]
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t) * 1e3 / a.steps
        assert torch.isfinite(out).all()
        return ms

    res = {"steps_ms": {}, "blend_pair_us": {}}
    for b in a.batches:
        for v in variants:                                    # warm-up: code objects, workspaces, the captured graph of the shape
            one(b, v)
        runs = {v: [] for v in variants}
        for _ in range(a.repeats):
            for v in variants:
                runs[v].append(one(b, v))
        res["steps_ms"][str(b)] = runs
        if hasattr(ops, "inpaint_in"):
            x, lat, noise = (torch.randn(b, 4, H, W, device="cuda:0") for _ in range(3))
            m = torch.rand(b, 1, H, W, device="cuda:0")
            sigma = torch.full((b,), 1.5, device="cuda:0")
            out = torch.empty_like(x)
            pair = lambda: (ops.inpaint_in(x, m, lat, noise, sigma, out=out), ops.inpaint_out_(out, m, lat))
            for _ in range(20):
                pair()
            n = 400
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            s.record()
            for _ in range(n):
                pair()
            e.record()
            torch.cuda.synchronize()
            res["blend_pair_us"][str(b)] = s.elapsed_time(e) * 1e3 / n
    print("INPAINT_COST " + json.dumps(res))


def spawn(a, root, variants):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--package-root", root, "--variants", ",".join(variants), "--steps", str(a.steps),
           "--repeats", str(a.repeats), "--batches"] + [str(b) for b in a.batches]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.child_timeout)
    if r.returncode != 0:
        raise SystemExit(f"the child for {root} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    line = [l for l in r.stdout.splitlines() if l.startswith("INPAINT_COST ")][-1]
    return json.loads(line[len("INPAINT_COST "):])


def summary(xs):
    return {"median_ms": statistics.median(xs), "min_ms": min(xs), "max_ms": max(xs), "runs": len(xs)}


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built: its unmasked step is measured too")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inpaint_cost.json"))
    ap.add_argument("--child-timeout", type=int, default=420)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--package-root", default=ROOT)
    ap.add_argument("--variants", default="unmasked,masked,masked_dd")
    return ap.parse_args(argv)


def measure(a, spawn=spawn):
    """The rounds: (this tree's runs, the parent tree's unmasked runs, the blend pair's times), per batch."""
    mine = {str(b): {v: [] for v in ("unmasked", "masked", "masked_dd")} for b in a.batches}
    parent = {str(b): [] for b in a.batches}
    pair = {}
    for _ in range(a.rounds):                                 # the trees alternate, one process with the device at a time
        if a.parent_tree:
            r = spawn(a, a.parent_tree, ["unmasked"])
            for b, runs in r["steps_ms"].items():
                parent[b] += runs["unmasked"]
        r = spawn(a, ROOT, ["unmasked", "masked", "masked_dd"])
        for b, runs in r["steps_ms"].items():
            for v, xs in runs.items():
                mine[b][v] += xs
        for b, us in r["blend_pair_us"].items():
            pair.setdefault(b, []).append(us)
    return mine, parent, pair


def report(a, mine, parent, pair):
    res = {"what": f"ms per sampler step through nodes.KSampler2, {H} x {W} latents, SD1.5-sized synthetic weights, {SAMPLER} / {SCHEDULER}, cfg {CFG}, "
                   f"{a.steps} steps a run", "rounds": a.rounds, "repeats_per_round": a.repeats, "batches": {},
           "how": "a fresh process per tree and round, the trees alternating; every shape warmed up, the variants alternating run by run; a run = host "
                  "clock around KSampler2().sample between device synchronises, over its steps; blend pair = HIP events around 400 back-to-back "
                  "inpaint_in + inpaint_out_ launches, per pair"}
    for b in mine:
        row = {v: summary(xs) for v, xs in mine[b].items()}
        base = row["unmasked"]["median_ms"]
        row["masked_minus_unmasked_ms"] = row["masked"]["median_ms"] - base
        row["masked_minus_unmasked_percent"] = 100.0 * row["masked_minus_unmasked_ms"] / base
        row["masked_dd_minus_unmasked_ms"] = row["masked_dd"]["median_ms"] - base
        row["masked_dd_minus_unmasked_percent"] = 100.0 * row["masked_dd_minus_unmasked_ms"] / base
        row["blend_pair_us"] = statistics.median(pair[b])
        if a.parent_tree:
            row["parent_unmasked"] = summary(parent[b])
            row["unmasked_minus_parent_unmasked_ms"] = base - row["parent_unmasked"]["median_ms"]
        res["batches"][b] = row
    return res


def main(argv=None):
    a = parse(argv)
    if a.child:
        return child(a)
    res = report(a, *measure(a))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
