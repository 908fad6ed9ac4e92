"""The TAESD executor (csrc/taesd.hip taesd_run) against a chain of operator calls (tests/taesd_chain.py), per launch and per bit; every stage
of the chain element-wise against fp64 on the operands the network really feeds it.

B1  same launches: the chain's launch list (ops.last_launches() of every call) equals the executor's launch table (profile_launches after
    profile), entry by entry; a mismatch names the first differing layer.  35 launches; taesd_conv_kernel<up> three times, at 10, 20, 30.
B2  same bits: torch.equal(executor, chain) on the fp32 decode AND on the uint8 image for every case — also with every other case run in
    between on the same handle (A, B, A), on a fresh handle that had to grow its workspace for the case, and under the graph that
    LatentPreviewer(use_graph=True) captures and replays.  No tolerance.  Layers held under an exception instead: none.
B3  every stage element-wise, on ALL rows: for each tap the fp64 reference of that one stage from the stage's own inputs and the bounds that
    exist — taesd_conv_ref (tests/test_taesd_conv_gpu.py), EB.taesd_first_ref, EB.taesd_last_ref — through EB.check with the signed-bias
    statistic (EB.rtn_noise on top below 10^4 elements: chain_harness.held).  What only the executor reaches: three buffers
    that rotate through four resolutions, a Block's third convolution writing over t1 with the Block's input as residual, the bias-free
    up-convolution from the old size into the next buffer at the new one.  The largest fp64 im2col is 136 x 264 x 576 (165 MB).
    With LD_WRITE_PARITY=1 the worst error / bound and signed bias per stage kind and case go to profiles/taesd_chain_parity.json (a record).
B4  the chain is the reference's network: on the taesd_9x13 / taesd_b2_17x33 fixtures it meets the allowances of tests/test_preview_gpu.py
    unchanged (twice the fixture's emulation distances; the image within ceil(255 emul_max_abs) counts).

Cases: the smallest shapes that reach each path (the halo tile is 16 x 32 output pixels), each with latents randn x 1 and randn x 4 (the
Clamp saturates, as in tests/test_preview_gpu.py).
"""
import json
import math

import pytest
import torch

import chain_harness as H
import errbound as EB
import taesd_ref as TR
from conftest import load_golden, rel_l2
from test_taesd_conv_gpu import taesd_conv_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAUNCHES = 35

SHAPES = {"1_3x5": (1, 3, 5),          # the smallest; 1/8 .. 1/2 resolution under one tile
          "3_2x2": (3, 2, 2),          # odd batch
          "2_9x13": (2, 9, 13),        # a golden shape, a batch of two
          "1_17x33": (1, 17, 33)}      # a golden shape: every resolution over a tile
# name -> ((n, h, w), latent scale)
CASES = {f"{k}_x{s}": (shape, float(s)) for k, shape in SHAPES.items() for s in (1, 4)}


def inputs(name):
    (n, h, w), scale = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    return (torch.randn(n, 4, h, w, generator=g) * scale).to(DEV)


def _fresh(seed=0):
    from lightdiffusion_amd import nodes as N
    return N.load_synthetic_taesd(DEV, seed=seed, max_hw=(2, 2), max_batch=1)


class Side:
    """The executor's handle, the chain, and per case the chain's outputs and taps (computed once, never changed)."""

    def __init__(self):
        from taesd_chain import TAESDChain
        self.model = _fresh()                              # every case's first run grows the workspace
        self.chain = TAESDChain(DEV)
        self._chain_runs = {}

    def chain_run(self, name):
        if name not in self._chain_runs:
            out, img = self.chain.decode(inputs(name))
            self._chain_runs[name] = (out, img, self.chain.taps)
        return self._chain_runs[name]

    def executor_run(self, name, model=None):
        got, img = (model or self.model)._run(inputs(name), True)
        assert img.dtype == torch.uint8, img.dtype
        return got, img

    def executor_table(self, name):
        return [r[4] for r in self.model.profile(inputs(name))]


@pytest.fixture(scope="module")
def side():
    s = Side()
    yield s
    del s
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ B1

@pytest.mark.parametrize("name", list(CASES))
def test_same_launches(side, name):
    from taesd_chain import modules
    _, _, taps = side.chain_run(name)
    mine = H.same_launches(name, taps, side.executor_table(name))
    assert len(mine) == len(taps) == side.model.last_launches == LAUNCHES
    assert [(t["kind"], t["name"]) for t in taps] == [(k, nm) for k, nm, _, _ in modules()]
    names = [k for _, k in mine]
    assert names[0] == "taesd_first_kernel" and names[-1] == "taesd_last_kernel"
    assert names.count("taesd_conv_kernel<up>") == 3 and [i for i, k in enumerate(names) if k == "taesd_conv_kernel<up>"] == [10, 20, 30]
    assert names.count("taesd_conv_kernel") == 30
    (n, h, w), _ = CASES[name]
    ups = [t for t in taps if t["kind"] == "up"]
    assert [tuple(t["out"].shape) for t in ups] == [(n, h << k, w << k, 64) for k in (1, 2, 3)]
    assert all(t["par"]["b"] is None for t in ups) and all(t["par"]["b"] is not None for t in taps if t["kind"] != "up")


# ------------------------------------------------------------------ B2

@pytest.mark.parametrize("name", list(CASES))
def test_same_bits(side, name):
    want, want_img, _ = side.chain_run(name)
    assert bool(torch.isfinite(want).all()), f"{name}: the chain read an element nobody wrote"
    assert torch.equal(want_img, TR.to_image(want)), "the image is not the formula on the chain's own decode"
    n, h, w = shape = CASES[name][0]
    H.same_bits(name, (want, want_img), side.executor_run, [o for o in CASES if CASES[o][0] != shape])      # the decode and the image; A, B, A on the one handle
    grown = _fresh()                                       # a handle that has to grow its workspace for this case
    before = grown.workspace_bytes
    got = side.executor_run(name, grown)
    assert grown.workspace_bytes > before and grown.workspace_bytes == grown.plan_bytes(n, h, w)
    H.bits_held(got, (want, want_img), f"{name} on a grown workspace")


@pytest.mark.parametrize("name", list(CASES))
def test_same_bits_under_the_previewer_graph(side, name):
    from lightdiffusion_amd.preview import LatentPreviewer
    want, want_img, _ = side.chain_run(name)
    n = CASES[name][0][0]
    got = []
    pv = LatentPreviewer(side.model, lambda i, im: got.append(im), rows=slice(0, n), use_graph=True)
    x = inputs(name)
    for i in range(2):                                     # the capture's replay, and a second replay
        pv({"x": x, "i": i, "sigma": 1.0, "denoised": None})
        assert pv._graph is not None
        H.bits_held((pv._f32, got[-1]), (want, want_img.cpu()), f"{name} replay {i}")


# ------------------------------------------------------------------ B3

def _stage(tap, what):
    """[(error / bound, signed bias)] of one tap's output against the fp64 reference of that stage."""
    kind, i, p, out = tap["kind"], tap["inp"], tap["par"], tap["out"]
    n, h, w, _ = out.shape
    where = dict(image_rows=h * w, width=w)
    if kind == "first":
        ref, bound = EB.taesd_first_ref(i["x"], p["w"], p["b"])
        assert float(out.min()) >= 0.0
        return [H.held(out.reshape(-1, 64), ref, bound, what, keep=ref > 0, **where)]
    if kind == "last":
        ref, bound, img_ref = EB.taesd_last_ref(i["x"], p["w"], p["b"])
        img = tap["image"]
        assert torch.equal(img, TR.to_image(out)), f"{what}: the image is not the formula on the device's own decode"
        off = (img.reshape(-1, 3).long() - img_ref.long()).abs()
        assert int(off.max()) <= 1, f"{what}: image byte {int(off.max())} counts from the fp64 reference's"
        return [H.held(out.reshape(-1, 3), ref, bound, what, keep=torch.ones_like(ref, dtype=torch.bool), **where)]
    assert (kind == "up") == p["up"] and (p["b"] is None) == (kind == "up")
    ref, bound = taesd_conv_ref(i["x"], p["w"], p["b"], i["residual"], p["relu"], p["up"])
    if p["relu"]:
        assert float(out.min()) >= 0.0
    return [H.held(out.reshape(-1, 64), ref, bound, what, **where)]


@pytest.mark.parametrize("name", list(CASES))
def test_every_stage_elementwise(side, name):
    _, _, taps = side.chain_run(name)
    rec, fails = H.every_stage(name, taps, _stage)
    print(f"PARITY {name}: " + json.dumps(rec))
    H.record("taesd_chain_parity.json", name, rec)
    H.stages_held(fails, taps)


# ------------------------------------------------------------------ B4

@pytest.mark.parametrize("fixture", ["taesd_9x13", "taesd_b2_17x33"])
def test_chain_meets_the_goldens(fixture):
    from taesd_chain import TAESDChain
    g = load_golden(fixture)
    d, img = TAESDChain(DEV, seed=int(g["weight_seed"])).decode(g["x"])
    d, img = d.cpu(), img.cpu()
    assert d.shape == g["y"].shape and img.shape == g["image"].shape
    err, allow = rel_l2(d, g["y"]), 2.0 * float(g["emul_rel_l2"])
    mx, mallow = float((d - g["y"]).abs().max()), 2.0 * float(g["emul_max_abs"])
    counts, callow = int((img.int() - g["image"].int()).abs().max()), math.ceil(255.0 * float(g["emul_max_abs"]))
    print(f"{fixture}: chain rel-L2 {err:.3e} (allowance {allow:.3e}), max-abs {mx:.3e} (allowance {mallow:.3e}), image {counts} counts (allowance {callow})")
    H.record("taesd_chain_parity.json", "fixture " + fixture, {"chain_rel_l2": round(err, 7), "allowance": round(allow, 7), "chain_max_abs": round(mx, 6),
                                                               "max_abs_allowance": round(mallow, 6)})
    assert err <= allow and mx <= mallow and counts <= callow, (err, allow, mx, mallow, counts, callow)
