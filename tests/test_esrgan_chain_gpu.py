"""The ESRGAN executor (csrc/esrgan.hip esrgan_run) against a chain of operator calls (tests/esrgan_chain.py), per launch and per bit; every
stage of the chain element-wise against fp64 on the operands the network really feeds it.

B1  same launches: the chain's launch list (ops.last_launches() of every call) equals the executor's launch table (profile_launches after
    profile), entry by entry; a mismatch names the first differing layer.  15 nb + 4 + log2(scale) launches (15 nb + 6 at x4, the shipped
    scale).  REACHES: what each case is in the table for.
B2  same bits: torch.equal(executor, chain) on forward_device for every case — also with every other case of the config run in between on
    the same handle (A, B, A: the tiled upscaler runs one handle at many sizes in a row), and on a fresh handle that had to grow its
    workspace for the case.  No tolerance.  Layers held under an exception instead: none.
B3  every stage element-wise, on ALL rows: for each tap the fp64 reference of that one stage from the stage's own fp16 inputs and the bounds
    that exist — dense_conv_ref (tests/test_esrgan_conv_gpu.py), EB.esrgan_first_ref, EB.esrgan_last_ref — through EB.check with the
    signed-bias statistic (EB.rtn_noise on top below 10^4 elements: chain_harness.held).  What only the executor reaches: the
    in-place append into a buffer with stale channels (every channel outside [c_off, c_off + cout) bit-unchanged), convolution 5's R1 out
    of its own input buffer, the second store y2 over R2 (y2 == the stored y, bit for bit), the trunk convolution's buffer by the parity
    of 3 nb, the HR convolution on the pitch-192 buffer at scale 1, three up-convolutions at scale 8.
    With LD_WRITE_PARITY=1 the worst error / bound and signed bias per stage kind and case go to profiles/esrgan_chain_parity.json (a record).
B4  the chain is the reference's network: on the esrgan_x4_nb2 / esrgan_x2_nb1 fixtures it meets the allowance of tests/test_upscale_gpu.py
    unchanged (twice the fixture's emulation distance); the scale-1 and scale-8 configs, which have no fixture, against esrgan_ref.rrdbnet
    in fp32 on the CPU with an allowance measured as the fixtures' was: twice the rel-L2 of rrdbnet(emulate_fp16=True) from the fp32 run
    (tests/test_upscale_cpu.py pins that mode against the fixtures).  Nothing of an allowance comes from device output.

Cases: the smallest shapes that reach each path (the halo tile is 16 x 32 output pixels); images are rand in [0, 1].
"""
import json

import pytest
import torch

import chain_harness as H
import errbound as EB
import esrgan_ref as ER
from conftest import load_golden, rel_l2
from lightdiffusion_amd import weights as W
from test_esrgan_conv_gpu import dense_conv_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

CONFIGS = {"x2nb1": (1, 2), "x4nb2": (2, 4), "x1nb1": (1, 1), "x8nb1": (1, 8)}          # tag -> (nb, scale)
# name -> (config, (n, h, w))
CASES = {
    "x2nb1_1_5x7": ("x2nb1", (1, 5, 7)),          # odd swap count (3): the trunk reads dense[1]; under one tile
    "x2nb1_2_9x11": ("x2nb1", (2, 9, 11)),        # batch borders; A, B, A
    "x4nb2_1_17x33": ("x4nb2", (1, 17, 33)),      # even swap count (6): the trunk reads dense[0]; one row and one column over the tile; golden config
    "x4nb2_3_4x6": ("x4nb2", (3, 4, 6)),          # odd batch
    "x1nb1_2_6x10": ("x1nb1", (2, 6, 10)),        # no up-convolution: the HR convolution reads the pitch-192 buffer
    "x1nb1_1_17x9": ("x1nb1", (1, 17, 9)),
    "x8nb1_1_3x5": ("x8nb1", (1, 3, 5)),          # three up-convolutions; the arena grows per stage
}
UP = "esrgan_conv_kernel<64,up>"
# kernel name -> how often the case's launch list must hold it
REACHES = {name: {UP: ER.n_upconvs(CONFIGS[tag][1]), "esrgan_conv_kernel<32>": 12 * CONFIGS[tag][0], "esrgan_conv_kernel<64>": 3 * CONFIGS[tag][0] + 2,
                  "esrgan_first_kernel": 1, "esrgan_last_kernel": 1} for name, (tag, _) in CASES.items()}


def config(tag):
    nb, scale = CONFIGS[tag]
    return W.esrgan_config(nb, scale)


def inputs(name):
    n, h, w = CASES[name][1]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    return torch.rand(n, h, w, 3, generator=g).to(DEV)


def _gen(name, shape):
    return W.synth_tensor(name, shape, 0)


class Side:
    """One config: the executor's handle, the chain, and per case the chain's output and taps (computed once, never changed)."""

    def __init__(self, tag):
        from esrgan_chain import ESRGANChain
        from lightdiffusion_amd.upscale import MI355XUpscaler
        self.tag, self.cfg = tag, config(tag)
        self.model = MI355XUpscaler(self.cfg, _gen, device=DEV, max_batch=1, max_hw=(2, 2))      # every case's first run grows the workspace
        self.chain = ESRGANChain(self.cfg, DEV)
        self._chain_runs = {}

    def chain_run(self, name):
        if name not in self._chain_runs:
            out = self.chain.forward(inputs(name))
            self._chain_runs[name] = (out, self.chain.taps)
        return self._chain_runs[name]

    def executor_run(self, name):
        return self.model.forward_device(inputs(name))

    def executor_table(self, name):
        return [r[4] for r in self.model.profile(inputs(name))]


side = H.side_fixture(Side)


# ------------------------------------------------------------------ B1

@pytest.mark.parametrize("name", list(CASES))
def test_same_launches(side, name):
    from esrgan_chain import modules
    tag = CASES[name][0]
    s = side(tag)
    nb, scale = CONFIGS[tag]
    _, taps = s.chain_run(name)
    mine = H.same_launches(name, taps, s.executor_table(name))
    assert len(mine) == len(taps) == s.model.last_launches == 15 * nb + 4 + ER.n_upconvs(scale), (len(mine), len(taps), s.model.last_launches)
    assert [(t["kind"], t["name"]) for t in taps] == [(k, nm) for k, nm, _, _ in modules(s.cfg)]
    names = [k for _, k in mine]
    print(f"LAUNCHES {name}: {sorted(set(names))}")
    for kernel, count in REACHES[name].items():
        assert names.count(kernel) == count, f"{name} was to run {kernel} {count} times, not {names.count(kernel)}: {names}"
    assert sum(REACHES[name].values()) == len(names)
    y2 = [t["name"] for t in taps if t["kind"] == "conv5" and t["y2"] is not None]
    assert y2 == [f"model.1.sub.{b}.RDB3.conv5.0" for b in range(nb)], y2            # the second store: every RRDB's third block, nowhere else
    if scale == 1:                                                                     # the HR convolution on the pitch-192 buffer
        hr = next(t for t in taps if t["kind"] == "hr")
        trunk = next(t for t in taps if t["kind"] == "trunk")
        assert trunk["after"].shape[-1] == 192 and torch.equal(hr["inp"]["x"], trunk["out"])


# ------------------------------------------------------------------ B2

@pytest.mark.parametrize("name", list(CASES))
def test_same_bits(side, name):
    from lightdiffusion_amd.upscale import MI355XUpscaler
    tag = CASES[name][0]
    s = side(tag)
    want, _ = s.chain_run(name)
    assert bool(torch.isfinite(want).all()), f"{name}: the chain read a channel nobody wrote"
    H.same_bits(name, want, s.executor_run, [o for o in CASES if o != name and CASES[o][0] == tag])      # shape history A, B, A on the one handle
    n, h, w = CASES[name][1]
    grown = MI355XUpscaler(s.cfg, _gen, device=DEV, max_batch=1, max_hw=(2, 2))       # a handle that has to grow its workspace for this case
    before = grown.workspace_bytes
    got = grown.forward_device(inputs(name))
    assert grown.workspace_bytes > before and grown.workspace_bytes == grown.plan_bytes(n, h, w)
    H.bits_held(got, want, f"{name} on a grown workspace")


# ------------------------------------------------------------------ B3

def _bits(t):
    return t.contiguous().view(torch.int16)


def _stage(tap, what):
    """[(error / bound, signed bias)] of one tap's output against the fp64 reference of that stage; the stage's buffer contract bit for bit."""
    kind, i, p, out = tap["kind"], tap["inp"], tap["par"], tap["out"]
    if kind == "last":
        n, h, w, _ = i["x"].shape
        ref, bound = EB.esrgan_last_ref(i["x"], p["w"], p["b"])
        return [H.held(out.reshape(-1, 3), ref, bound, what, keep=torch.ones_like(ref, dtype=torch.bool), image_rows=h * w, width=w)]
    c_off, cout = p["c_off"], p["cout"]
    before, after = tap["before"], tap["after"]
    n, h, w, ld = after.shape
    outside = torch.ones(ld, dtype=torch.bool, device=after.device)
    outside[c_off:c_off + cout] = False
    assert torch.equal(_bits(after)[..., outside], _bits(before)[..., outside]), f"{what}: channels outside [{c_off}, {c_off + cout}) changed"
    assert torch.equal(_bits(after[..., c_off:c_off + cout]), _bits(out))
    if tap["y2"] is not None:
        assert torch.equal(_bits(tap["y2"][..., :cout]), _bits(out)), f"{what}: the second store differs from y"
        assert tap["y2"].shape[-1] == cout
    if kind == "first":
        assert tap["y2"] is not None
        ref, bound = EB.esrgan_first_ref(i["x"], p["w"], p["b"])
    else:
        res = [(s, r) for s, r in ((p["s1"], i["r1"]), (p["s2"], i["r2"])) if r is not None]
        ref, bound = dense_conv_ref(i["x"], p["w"], p["b"], p["slope"], res, up=p["up"])
    return [H.held(out.reshape(-1, cout), ref, bound, what, image_rows=h * w, width=w)]


@pytest.mark.parametrize("name", list(CASES))
def test_every_stage_elementwise(side, name):
    s = side(CASES[name][0])
    _, taps = s.chain_run(name)
    rec, fails = H.every_stage(name, taps, _stage)
    print(f"PARITY {name}: " + json.dumps(rec))
    H.record("esrgan_chain_parity.json", name, rec)
    H.stages_held(fails, taps)


# ------------------------------------------------------------------ B4

@pytest.mark.parametrize("fixture", ["esrgan_x4_nb2", "esrgan_x2_nb1"])
def test_chain_meets_the_goldens(side, fixture):
    g = load_golden(fixture)
    tag = {(2, 4): "x4nb2", (1, 2): "x2nb1"}[(int(g["nb"]), int(g["scale"]))]
    assert int(g["weight_seed"]) == 0
    y = side(tag).chain.forward(g["x"]).cpu()
    assert y.shape == g["y"].shape
    err, allow = rel_l2(y, g["y"]), 2.0 * float(g["emul_rel_l2"])
    print(f"{fixture}: chain rel-L2 {err:.3e} (allowance {allow:.3e})")
    H.record("esrgan_chain_parity.json", "fixture " + fixture, {"chain_rel_l2": round(err, 7), "allowance": round(allow, 7)})
    assert err <= allow, (err, allow)


@pytest.mark.parametrize("name", [n for n, (tag, _) in CASES.items() if tag in ("x1nb1", "x8nb1")])
def test_chain_meets_the_restatement_without_a_fixture(side, name):
    """Scale 1 and scale 8: against esrgan_ref.rrdbnet in fp32 on the CPU; the allowance is twice the distance of the fp16 emulation of the
    same restatement from that fp32 run (same rounding points as the kernels, another summation order: the fixtures' margin)."""
    tag = CASES[name][0]
    nb, scale = CONFIGS[tag]
    s = side(tag)
    x = inputs(name).cpu()
    sd = W.synth_state_dict(W.esrgan_param_shapes(s.cfg), 0)
    ref = ER.rrdbnet(sd, x, nb, scale)
    emul = rel_l2(ER.rrdbnet(sd, x, nb, scale, emulate_fp16=True), ref)
    out, _ = s.chain_run(name)
    err, allow = rel_l2(out.cpu(), ref), 2.0 * emul
    print(f"{name}: chain rel-L2 {err:.3e}, emulation {emul:.3e} (allowance {allow:.3e})")
    H.record("esrgan_chain_parity.json", name, {"vs_fp32_restatement": {"chain_rel_l2": round(err, 7), "emulation_rel_l2": round(emul, 7), "allowance": round(allow, 7)}})
    assert out.shape == ref.shape and err <= allow, (err, emul, allow)
