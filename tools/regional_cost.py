"""What regional conditioning costs per step: ms per sampler step through nodes.KSampler2 at 64 x 64 latents (512^2 images),
batch 1 and batch 8, SD1.5-sized synthetic weights, dpmpp_2m_sde / karras, for
  plain          (a) single unkeyed conditioning, no option: the replayed-graph route every existing caller takes
  multi_off      (b) two masked positives + one negative, option off: the multi-entry eager route (the keys inert; the parent runs this too)
  one_group      (c) the same lists with apply_cond_areas=True: one group of three whole-latent entries; gather + combine in place of the
                     torch cat / chunk / stack / sum / divide of (b)
  three_groups   (d) a whole entry + two areas of different shapes (and their negative partners): three groups, three eager UNet calls a step,
                     the context re-projected per group
and, with --parent-tree DIR (a checkout of the parent commit with its library built), the parent's (a) and (b) on the same box in the same
session.  Every tree is measured in a fresh child process of its own, one at a time, the trees alternating (--rounds); inside a process every
shape is warmed up first and the variants alternate run by run.  What is compared ACROSS trees is measured in processes that do the same work:
per round the parent's (a) + (b), then this tree's (a) + (b) in a process of exactly that sequence, then this tree's (b) + (c) + (d) in a third
(measured once with all four cases alternating in one process, (a) at batch 8 read 70 us above the parent's, whose process ran (a) + (b) only:
what runs between two runs of a case is part of what is measured).  A run is timed with a host clock around KSampler2().sample between two
device synchronises (the call ends with the samples on the host) and divided by its steps; the figure per variant is the median over all runs,
with the minimum and maximum beside it.  (e) the gather + combine pair of (c) is also timed on its own: HIP events around a few hundred back-to-back pairs.

Acceptance (recorded in the output, not gated by pytest): (a) on this tree lies within the parent's own spread (its minimum to its maximum over
the alternated rounds); (c) is not slower than the parent's (b) by more than that spread.

    python tools/regional_cost.py [--parent-tree DIR] [--steps 20] [--repeats 4] [--rounds 2] [--out profiles/regional_cost.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = W = 64
SAMPLER, SCHEDULER, CFG = "dpmpp_2m_sde", "karras", 7.0
PARENT = ("plain", "multi_off")                               # what both trees run, in processes of the same sequence
NEW = ("multi_off", "one_group", "three_groups")              # this tree's second process: (b) again beside (c) and (d)
MINE = ("plain", "multi_off", "one_group", "three_groups")
AREAS = ((32, 64, 0, 0), (64, 32, 0, 32))                     # (d): (h, w, y, x) on the latent, two shapes


def toks(word):
    return [[(49406, 1.0)] + [(word, 1.0)] * 3 + [(49407, 1.0)] * 73]


def child(a):
    """One tree, one process: {batch: {variant: [ms per step, ...]}} (and the kernel pair's time) as one JSON line on stdout."""
    sys.path.insert(0, os.path.abspath(a.package_root))
    import torch
    from lightdiffusion_amd import nodes as N
    from lightdiffusion_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("regional_cost.py measures on the GPU; none is visible")
    variants = a.variants.split(",")
    # the workspaces are sized for the largest eager batch: three entries a group
    model, clip, _ = N.load_synthetic("cuda:0", max_batch=2 * max(a.batches), max_hw=(H, W))
    enc = lambda t: [[c, {"pooled_output": p}] for c, p in [clip.encode_from_tokens(t, return_pooled=True)]]
    p0, p1, p2, neg = enc(toks(320)), enc(toks(530)), enc(toks(1125)), enc(toks(2368))
    keyed = lambda c, **keys: [[t, dict(d, **keys)] for t, d in c]
    left = torch.zeros(1, H, W)
    left[:, :, : W // 2] = 1.0
    masked = keyed(p1, mask=left, mask_strength=1.0) + keyed(p2, mask=1.0 - left, mask_strength=1.0)
    areas = p0 + keyed(p1, area=AREAS[0], strength=1.0) + keyed(p2, area=AREAS[1], strength=1.0)
    conds = {"plain": (p0, {}), "multi_off": (masked, {}), "one_group": (masked, {"apply_cond_areas": True}),
             "three_groups": (areas, {"apply_cond_areas": True})}

    def one(b, variant):
        pos, kw = conds[variant]
        lat = {"samples": torch.zeros(b, 4, H, W)}
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = N.KSampler2().sample(model, 0, a.steps, CFG, SAMPLER, SCHEDULER, pos, neg, lat, **kw)[0]["samples"]
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t) * 1e3 / a.steps
        assert torch.isfinite(out).all()
        return ms

    res = {"steps_ms": {}, "kernel_pair_us": {}}
    for b in a.batches:
        for v in variants:                                    # warm-up: code objects, workspaces, the captured graph of the shape
            one(b, v)
        runs = {v: [] for v in variants}
        for _ in range(a.repeats):
            for v in variants:
                runs[v].append(one(b, v))
        res["steps_ms"][str(b)] = runs
        if hasattr(ops, "regional_combine"):
            x = torch.randn(b, 4, H, W, device="cuda:0")
            m = left.to("cuda:0")
            whole = (H, W, 0, 0)
            entries = [ops.RegionalEntry(1, 0, 0, whole), ops.RegionalEntry(0, 0, 1, whole, 1.0, (1.0 - m).contiguous(), 1.0),
                       ops.RegionalEntry(0, 0, 2, whole, 1.0, m, 1.0)]
            gat, out = torch.empty(3 * b, 4, H, W, device="cuda:0"), torch.empty_like(x)
            pair = lambda: (ops.regional_gather(x, [whole] * 3, out=gat), ops.regional_combine([gat], entries, CFG, x.shape, out=out))
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
            res["kernel_pair_us"][str(b)] = s.elapsed_time(e) * 1e3 / n
    print("REGIONAL_COST " + json.dumps(res))


def spawn(a, root, variants):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--package-root", root, "--variants", ",".join(variants), "--steps", str(a.steps),
           "--repeats", str(a.repeats), "--batches"] + [str(b) for b in a.batches]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.child_timeout)
    if r.returncode != 0:
        raise SystemExit(f"the child for {root} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    line = [l for l in r.stdout.splitlines() if l.startswith("REGIONAL_COST ")][-1]
    return json.loads(line[len("REGIONAL_COST "):])


def summary(xs):
    return {"median_ms": statistics.median(xs), "min_ms": min(xs), "max_ms": max(xs), "runs": len(xs)}


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built: its (a) and (b) are measured too")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regional_cost.json"))
    ap.add_argument("--child-timeout", type=int, default=420)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--package-root", default=ROOT)
    ap.add_argument("--variants", default=",".join(MINE))
    return ap.parse_args(argv)


def measure(a, spawn=spawn):
    """The rounds: (this tree's runs, the parent tree's runs, the kernel pair's times), per batch.  This tree's "multi_off" is the one measured
    beside "plain", as the parent's is; the one measured beside (c) and (d) is kept as "multi_off_beside_new"."""
    mine = {str(b): {v: [] for v in MINE + ("multi_off_beside_new",)} for b in a.batches}
    parent = {str(b): {v: [] for v in PARENT} for b in a.batches}
    pair = {}
    for _ in range(a.rounds):                                 # the trees alternate, one process with the device at a time
        if a.parent_tree:
            r = spawn(a, a.parent_tree, list(PARENT))
            for b, runs in r["steps_ms"].items():
                for v, xs in runs.items():
                    parent[b][v] += xs
        r = spawn(a, ROOT, list(PARENT))
        for b, runs in r["steps_ms"].items():
            for v, xs in runs.items():
                mine[b][v] += xs
        r = spawn(a, ROOT, list(NEW))
        for b, runs in r["steps_ms"].items():
            for v, xs in runs.items():
                mine[b]["multi_off_beside_new" if v == "multi_off" else v] += xs
        for b, us in r["kernel_pair_us"].items():
            pair.setdefault(b, []).append(us)
    return mine, parent, pair


def report(a, mine, parent, pair):
    res = {"what": f"ms per sampler step through nodes.KSampler2, {H} x {W} latents, SD1.5-sized synthetic weights, {SAMPLER} / {SCHEDULER}, cfg {CFG}, "
                   f"{a.steps} steps a run", "rounds": a.rounds, "repeats_per_round": a.repeats, "batches": {},
           "cases": {"plain": "(a) single unkeyed conditioning: the graph route", "multi_off": "(b) two masked positives + one negative, option off",
                     "one_group": "(c) the same lists, apply_cond_areas=True: one group", "three_groups": "(d) a whole entry + two areas of different "
                     "shapes: three groups", "kernel_pair_us": "(e) regional_gather + regional_combine of (c) alone"},
           "how": "a fresh process per tree and round, the trees alternating; every shape warmed up, the variants alternating run by run; a run = host "
                  "clock around KSampler2().sample between device synchronises, over its steps; kernel pair = HIP events around 400 back-to-back "
                  "regional_gather + regional_combine launches, per pair"}
    for b in mine:
        row = {v: summary(xs) for v, xs in mine[b].items()}
        row["one_group_minus_multi_off_ms"] = row["one_group"]["median_ms"] - row["multi_off_beside_new"]["median_ms"]      # same process
        row["three_groups_minus_one_group_ms"] = row["three_groups"]["median_ms"] - row["one_group"]["median_ms"]
        row["extra_group_ms"] = row["three_groups_minus_one_group_ms"] / 2.0
        row["kernel_pair_us"] = statistics.median(pair[b])
        if a.parent_tree:
            pa, pb = summary(parent[b]["plain"]), summary(parent[b]["multi_off"])
            row["parent_plain"], row["parent_multi_off"] = pa, pb
            row["plain_minus_parent_plain_ms"] = row["plain"]["median_ms"] - pa["median_ms"]
            row["one_group_minus_parent_multi_off_ms"] = row["one_group"]["median_ms"] - pb["median_ms"]
            row["plain_within_parent_spread"] = pa["min_ms"] <= row["plain"]["median_ms"] <= pa["max_ms"]
            row["one_group_not_slower_than_parent_multi_off_by_more_than_its_spread"] = \
                row["one_group"]["median_ms"] <= pb["median_ms"] + (pb["max_ms"] - pb["min_ms"])
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
