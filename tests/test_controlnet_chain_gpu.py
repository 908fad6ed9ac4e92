"""ControlNet on the device (csrc/unet.hip in control mode, ld_unet_forward with an ld_control) against chains of operator calls: the control branch
against tests/controlnet_chain.py's ControlChain, the controlled UNet against tests/unet_chain.py's UNetChain.forward(control=...), per launch
and per bit; every stage of both chains element-wise against fp64.  Tiny configuration, and SD1.5's width at 16 x 16 (all 13 residuals at
C = 320 / 640 / 1280, from 16 x 16 down to 2 x 2).  The full-size cases: tests/test_controlnet_chain_full_gpu.py.

A case is (config, n or nb, (h, w), tokens, mode, hint batch, strength); mode "pair_rn2": the branch runs as `forward` on the nb latents
against the first nb rows of the context, and its residuals join the 2 nb samples of the UNet's pair with r_n = nb (sample s reads s % nb).

B1  same launches: the control chain's launch list equals the branch's launch table (ld_controlnet_profile), the controlled UNet
    chain's equals that of ld_unet_profile with the ld_control, entry by entry; and the controlled table IS the plain table with exactly one
    control_add_kernel entry behind the middle block's last launch (asserted on the tables).  The hint encoder has no table of its own
    (ld_controlnet_set_hint is no forward): its eight launches are held as a count — last_launches == 8 behind set_hint — against the
    chain's eight hint_conv_kernel launches.
B2  same bits: the encoded hint, all 13 residuals and the controlled output are torch.equal to the chains', also with every other case of the
    same config run in between on the same two handles (A, B, A: a smaller case behind a larger one reads residual buffers that hold the
    larger one's rows), and — the pair cases — under the replayed graph: unet.cfg_denoise(..., control=...), first contact and one replay,
    is ops.cfg_combine of the chain's pair output, the residuals in the handle the chain's.  No tolerance.  ("pair_rn2" has no sampler
    route: no graph lap.)
    Layers held under an exception instead: none.
B3  every stage: tests/test_unet_chain_gpu.py's `_stage` for every kind it knows (a zero convolution is a `conv` tap), and two more:
    `control_add`, the bits of (t.float() + strength * r[s % r_n].float()).half() on the tap's saved pre-add operands, and `hint_conv`,
    `hint_ref` and `held` of tests/test_control_ops_gpu.py.  No new bound.  The operands are what is new: conv_in sums with the hint on top,
    skip tensors with residuals of their own magnitude added.  With LD_WRITE_PARITY=1 the records go to profiles/controlnet_chain_parity.json.
B4  the chain is the network: on two tiny cases the control chain's residuals and the controlled chain's output meet tests/controlnet_ref.py
    under UNET_TOL = 5e-3 (the golden bound of tests/test_models_gpu.py), and control moves the output by more than 10 x that bound.
Completeness: the control chain reads exactly the parameters of W.controlnet_param_shapes; a chain with two residuals of equal shape swapped
    differs from the executor (B2 sees an ordering defect).
"""
import json

import pytest
import torch

import chain_harness as H
import test_control_ops_gpu as CO
import test_unet_chain_gpu as U
from conftest import rel_l2
from lightdiffusion_amd import weights as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
UNET_TOL = U.UNET_TOL
SCALE = 3.0
RECORD = "controlnet_chain_parity.json"

# name -> (config, n or nb, (h, w), tokens, mode, hint batch, strength)
CASES = {
    "tiny_2_8x12": ("tiny", 2, (8, 12), 77, "forward", 1, 1.0),
    "tiny_1_7x9": ("tiny", 1, (7, 9), 77, "forward", 1, 1.0),                # ragged stride 2: residuals of 7x9, 4x5, 2x3, 1x2
    "tiny_3_13x4": ("tiny", 3, (13, 4), 154, "forward", 3, 0.6),
    "tiny_pair1_8x8": ("tiny", 1, (8, 8), 77, "pair", 1, 1.0),
    "tiny_pair2_8x8": ("tiny", 2, (8, 8), 77, "pair", 2, 1.0),               # sample s reads hint s % 2
    "tiny_2_8x8_eps": ("tiny", 2, (8, 8), 77, "eps", 1, 1.0),
    "tiny_pair2_8x8_rn2": ("tiny", 2, (8, 8), 77, "pair_rn2", 1, 1.0),
    "sd15_pair1_16x16": ("sd15", 1, (16, 16), 77, "pair", 1, 1.0),
    "sd15_4_16x16": ("sd15", 4, (16, 16), 77, "forward", 1, 1.0),
}


def is_pair(mode):
    return mode in ("pair", "pair_rn2")


def inputs(name, cases=None):
    """x, sigma, ctx as tests/test_unet_chain_gpu.inputs draws them (the same generator, the same order), then the hint."""
    tag, nb, (h, w), tokens, mode, hb, _ = (cases or CASES)[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    n_all = 2 * nb if is_pair(mode) else nb
    x = (torch.randn(nb, 4, h, w, generator=g) * 3.0).to(DEV)
    sigma = torch.tensor([U.SIGMAS[i % len(U.SIGMAS)] for i in range(nb)], dtype=torch.float32, device=DEV)
    ctx = torch.randn(n_all, tokens, U.config(tag)["context_dim"], generator=g).to(DEV)
    hint = torch.rand(hb, 3, 8 * h, 8 * w, generator=g).to(DEV)
    return x, sigma, ctx, hint


class Side:
    """One config: the two handles (UNet, control branch), the two chains, and per case the chains' results — the tuple (encoded hint, 13
    residuals, controlled output) — and taps, computed once and never changed.  one_case_taps: as tests/test_unet_chain_gpu.Side."""

    def __init__(self, tag, cases=None, one_case_taps=False):
        from controlnet_chain import ControlChain
        from lightdiffusion_amd.controlnet import synthetic_controlnet
        from lightdiffusion_amd.unet import synthetic_unet
        from unet_chain import UNetChain
        self.tag, self.cfg = tag, U.config(tag)
        self.cases = CASES if cases is None else cases
        mine = [c for c in self.cases.values() if c[0] == tag]
        kw = dict(max_batch=max((2 if is_pair(c[4]) else 1) * c[1] for c in mine), max_hw=(max(c[2][0] for c in mine), max(c[2][1] for c in mine)),
                  max_tokens=max(c[3] for c in mine))
        self.unet, self.cnet = synthetic_unet(self.cfg, **kw), synthetic_controlnet(self.cfg, **kw)
        self.chain, self.cchain = UNetChain(self.cfg, DEV), ControlChain(self.cfg, DEV)
        self.one_case_taps = one_case_taps
        self._runs = {}

    def inputs(self, name):
        return inputs(name, self.cases)

    def branch_inputs(self, name):
        """what the control branch runs on: -> x, sigma, its context, pair?"""
        mode = self.cases[name][4]
        x, sigma, ctx, _ = self.inputs(name)
        return x, sigma, (ctx[:x.shape[0]].contiguous() if mode == "pair_rn2" else ctx), mode == "pair"

    # -- the chains
    def chain_run(self, name):
        """-> ((hint, residual 0 .. 12, output), {"hint" | "branch" | "unet": taps})"""
        if name not in self._runs or self._runs[name][1] is None:
            _, nb, _, _, mode, _, strength = self.cases[name]
            if self.one_case_taps:
                self._runs = {k: (o, None) for k, (o, _) in self._runs.items()}
                self.chain.taps = self.cchain.taps = self.cchain.hint_taps = []
            x, sigma, ctx, hint = self.inputs(name)
            _, _, bctx, bpair = self.branch_inputs(name)
            enc = self.cchain.set_hint(hint)
            hint_taps = self.cchain.hint_taps
            self.cchain.set_context(bctx)
            res = self.cchain.forward(x, sigma, pair=bpair)
            self.chain.set_context(ctx)
            out = self.chain.forward(x, sigma, eps_only=mode == "eps", pair=is_pair(mode), control=(res, res[0].shape[0], strength))
            want = (enc, *res, out)
            if name in self._runs:
                H.bits_held(want, self._runs[name][0], f"{name}: the chains, run again for their taps,")
            self._runs[name] = (want, dict(hint=hint_taps, branch=self.cchain.taps, unet=self.chain.taps))
        return self._runs[name]

    def chain_out(self, name):
        return self._runs[name][0] if name in self._runs else self.chain_run(name)[0]

    # -- the executors
    def run_branch(self, name, profile=False):
        x, sigma, bctx, bpair = self.branch_inputs(name)
        hint = self.inputs(name)[3]
        self.cnet.set_context(bctx)
        self.cnet.set_hint(hint)
        assert self.cnet.last_launches == 8, f"{name}: set_hint counted {self.cnet.last_launches} launches"
        enc = self.cnet.hint()
        fn = {(False, False): self.cnet.forward, (False, True): self.cnet.forward_pair, (True, False): self.cnet.profile,
              (True, True): self.cnet.profile_pair}[(profile, bpair)]
        fn(x, sigma)
        return enc

    def executor_run(self, name):
        _, _, _, _, mode, _, strength = self.cases[name]
        x, sigma, ctx, _ = self.inputs(name)
        enc = self.run_branch(name)
        res = self.cnet.residuals()
        self.unet.set_context(ctx)
        ctl = self.cnet.control(strength)
        if is_pair(mode):
            out = self.unet.forward_pair(x, sigma, control=ctl)
        else:
            out = self.unet.forward(x, sigma, control=ctl, eps_only=mode == "eps")
        return (enc, *res, out)

    def tables(self, name):
        """-> the launch tables [kernel] of the branch, of the controlled UNet and of the plain UNet, and where their microseconds went"""
        _, _, _, _, mode, _, strength = self.cases[name]
        x, sigma, ctx, _ = self.inputs(name)
        self.run_branch(name, profile=True)
        rows = {"branch": self.cnet.profile_launches()}
        self.unet.set_context(ctx)
        ctl = self.cnet.control(strength)
        (self.unet.profile_pair if is_pair(mode) else self.unet.profile)(x, sigma, control=ctl)
        rows["controlled_unet"] = self.unet.profile_launches()
        (self.unet.profile_pair if is_pair(mode) else self.unet.profile)(x, sigma)
        rows["plain_unet"] = self.unet.profile_launches()
        branch, controlled, plain = ([r[4] for r in rows[k]] for k in ("branch", "controlled_unet", "plain_unet"))
        cost = {"branch": cost_of(rows["branch"]), "controlled_unet": cost_of(rows["controlled_unet"])["us"], "plain_unet": cost_of(rows["plain_unet"])["us"],
                "control_add": cost_of([r for r in rows["controlled_unet"] if r[4] == "control_add_kernel"])["us"]}
        return branch, controlled, plain, cost


side = H.side_fixture(Side)


def group(tag, cases=CASES):
    return [n for n in cases if cases[n][0] == tag]


# ------------------------------------------------------------------ B1

def zero_conv_routes(taps):
    """[(layer, (n, H, W, C), kernel)] of the zero convolutions and middle_block_out"""
    return [(t["name"], tuple(t["out"].shape), t["launches"]) for t in taps if t["name"].startswith(("zero_convs.", "middle_block_out."))]


def launches_held(name, s, reaches, zero_routes):
    """zero_routes: [(count, kernel)], the kernels of the 13 zero convolutions in the order the branch runs them"""
    _, taps = s.chain_run(name)
    branch, controlled, plain, cost = s.tables(name)
    hint = [(t["name"], t["launches"]) for t in taps["hint"]]
    assert [k for _, k in hint] == ["hint_conv_kernel"] * 8, f"{name}: the hint encoder's launches {hint}"
    mine_b = H.same_launches(name + " (control branch)", taps["branch"], branch)
    mine_u = H.same_launches(name + " (controlled UNet)", taps["unet"], controlled)
    # the controlled table is the plain one with ONE control_add_kernel entry behind the middle block's last launch
    k = 1 + max(j for j, (layer, _) in enumerate(mine_u) if layer.startswith("middle_block."))
    assert controlled[k] == "control_add_kernel" and mine_u[k][0].startswith("control"), f"{name}: launch {k} behind the middle block is {mine_u[k]}"
    assert controlled[:k] + controlled[k + 1:] == plain, f"{name}: the controlled table without launch {k} is not the plain table"
    assert "control_add_kernel" not in plain and controlled.count("control_add_kernel") == 1 and branch.count("control_add_kernel") == 1
    assert branch.index("control_add_kernel") == 1 + branch.index("small_conv_in_kernel"), f"{name}: the hint joins behind conv_in"
    zc = zero_conv_routes(taps["branch"])
    assert len(zc) == s.cnet.residual_count + 1
    print(f"ZERO CONVS {name}: " + json.dumps([[layer, list(shape), kern] for layer, shape, kern in zc]))
    names = {k for _, k in mine_b} | {k for _, k in mine_u} | {k for _, k in hint}
    print(f"LAUNCHES {name}: {sorted(names)}")
    print(f"COST {name}: " + json.dumps(cost))
    H.record(RECORD, name, {"launch_table_us": cost, "zero_convolutions": [[layer, list(shape), kern] for layer, shape, kern in zc]})
    for want in reaches:
        assert any(k.startswith(want) for k in names), f"{name} no longer reaches {want}: {sorted(names)}"
    want_zero = [kern for count, kern in zero_routes for _ in range(count)]
    assert [kern for _, _, kern in zc] == want_zero, f"{name}: the zero convolutions run {[kern for _, _, kern in zc]}"


def cost_of(rows):
    """{kernel: [launches, microseconds]} of a profiled table and its total (HIP events around every launch: a record, not a measurement)"""
    per = {}
    for r in rows:
        e = per.setdefault(r[4], [0, 0.0])
        e[0] += 1
        e[1] = round(e[1] + r[3], 1)
    return {"launches": len(rows), "us": round(sum(r[3] for r in rows), 1), "per_kernel": per}


# what every case reaches (kernel name prefixes), and ZERO_ROUTES: the kernels of its 13 zero convolutions, both read off the printed tables
_ALWAYS = ("control_add_kernel", "hint_conv_kernel", "small_conv_in_kernel", "small_conv_out_kernel", "timestep_embed_kernel", "flash_attn2_kernel",
           "gn_apply_kernel", "gn_stats_kernel+gn_apply_kernel")
REACHES = {name: _ALWAYS + (("dup_halves_kernel",) if is_pair(CASES[name][4]) else ()) for name in CASES}
_DEEP = "gemm3_kernel<64,160,conv,deep>"
_SD15_16 = [(7, _DEEP), (6, _DEEP + "+splitk_reduce_kernel")]       # C = 320 / 640 on <= 32 tiles; C = 1280 (4 x 4, 2 x 2): K / 640 = 2 slices
ZERO_ROUTES = {name: _SD15_16 if CASES[name][0] == "sd15" else [(13, "gemm3_kernel<64,128,conv>")] for name in CASES}


@pytest.mark.parametrize("name", list(CASES))
def test_same_launches(side, name):
    launches_held(name, side(CASES[name][0]), REACHES[name], ZERO_ROUTES[name])


# ------------------------------------------------------------------ B2

def graph_laps(name, s, want):
    """the captured step of the sampler (CFGDenoiser with a control): first contact and one replay"""
    from lightdiffusion_amd import ops
    from lightdiffusion_amd.controlnet import ControlNet
    _, nb, (h, w), _, mode, _, strength = s.cases[name]
    x, sigma, ctx, hint = s.inputs(name)
    cn = ControlNet(s.cnet).set_cond_hint(hint, strength)
    mixed = ops.cfg_combine(want[-1], SCALE)
    s.unet._denoisers.clear()
    for lap in (0, 1):
        got = s.unet.cfg_denoise(x, sigma, ctx, SCALE, control=cn)
        assert all(d._graph is not None for d in s.unet._denoisers.values()) and len(s.unet._denoisers) == 1
        H.bits_held(got, mixed, f"{name} under the replayed graph, lap {lap}")
        H.bits_held(tuple(s.cnet.residuals()), tuple(want[1:-1]), f"{name} residuals under the replayed graph, lap {lap}")
    assert cn.encode_calls == 1
    s.unet._denoisers.clear()


@pytest.mark.parametrize("name", list(CASES))
def test_same_bits(side, name):
    tag, mode = CASES[name][0], CASES[name][4]
    s = side(tag)
    want, _ = s.chain_run(name)
    H.same_bits(name, want, s.executor_run, [o for o in group(tag) if o != name])
    if mode == "pair":
        graph_laps(name, s, want)


# ------------------------------------------------------------------ B3

def _stage(tap, chain, what):
    kind, i, p, out = tap["kind"], tap["inp"], tap["par"], tap["out"]
    if kind == "control_add":
        for j, (t0, r, got) in enumerate(zip(i["t"], i["r"], out)):
            assert r.shape[0] == p["r_n"] and t0.shape[0] % p["r_n"] == 0 and got.shape == t0.shape, f"{what}: segment {j} shapes"
            rr = r.float().repeat((t0.shape[0] // p["r_n"],) + (1,) * (r.dim() - 1))          # sample s reads residual s % r_n
            wanted = (t0.float() + p["strength"] * rr).half()
            assert torch.equal(got, wanted), f"{what}: segment {j}: {H.differs(got, wanted)}"
        return [(0.0, 0.0)]
    if kind == "hint_conv":
        x = i["x"]
        a = x.half().permute(0, 2, 3, 1).contiguous() if x.dtype == torch.float32 else x
        ref, bound = CO.hint_ref(a, p["w"], p["b"], p["stride"], p["silu"])
        return [CO.held(out, ref, bound, what, out.shape[2])]
    return U._stage(tap, chain, what)


KINDS = {"hint": {"hint_conv"},
         "branch": {"timestep", "linear", "conv_in", "control_add", "groupnorm", "conv", "gn_conv", "linear_ln", "attention"},
         "unet": {"timestep", "linear", "conv_in", "conv_out", "control_add", "groupnorm", "conv", "upconv", "gn_conv", "linear_ln", "attention"}}


def stages(name, s, images=None):
    """-> the record {chain: {stage kind: ...}}, the failures, the number of taps"""
    _, taps = s.chain_run(name)
    rec, fails, count = {}, [], 0
    for part, chain in (("hint", s.cchain), ("branch", s.cchain), ("unet", s.chain)):
        kinds = {t["kind"] for t in taps[part]} - {"dup"}
        assert kinds == KINDS[part], f"{name} {part}: stage kinds {sorted(kinds)}"
        r, f = H.every_stage(f"{name} {part}", taps[part], lambda tap, what, chain=chain: _stage(tap, chain, what), images=images)
        rec[part] = r
        fails += f
        count += len(taps[part])
    return rec, fails, count


@pytest.mark.parametrize("name", list(CASES))
def test_every_stage_elementwise(side, name):
    s = side(CASES[name][0])
    rec, fails, count = stages(name, s)
    print(f"PARITY {name}: " + json.dumps(rec))
    H.record(RECORD, name, rec)
    assert not fails, f"{len(fails)} of {count} stages outside their bound:\n" + "\n".join(fails[:12])


# ------------------------------------------------------------------ B4

@pytest.mark.parametrize("name", ["tiny_2_8x12", "tiny_3_13x4"])
def test_chains_meet_the_reference(side, name):
    import controlnet_ref as R
    from oracle import sd15_ref as O
    s = side("tiny")
    strength = CASES[name][6]
    want, _ = s.chain_run(name)
    x, sigma, ctx, hint = (t.cpu() for t in inputs(name))
    sd, cn_sd, ms = W.synth_state_dict(W.unet_param_shapes(s.cfg)), R.synth_state_dict(s.cfg), O.ModelSampling()
    ref = R.control_residuals(cn_sd, s.cfg, ms, x, sigma, ctx, hint)
    got = [r.float().permute(0, 3, 1, 2).cpu() for r in want[1:-1]]
    assert len(got) == len(ref) == s.cnet.residual_count + 1
    errs = [rel_l2(g, r) for g, r in zip(got, ref)]
    print("residual rel-L2:", ["%.2e" % e for e in errs])
    assert max(errs) < UNET_TOL, errs
    out = want[-1].cpu()
    err = rel_l2(out, R.apply_model(sd, s.cfg, ms, x, sigma, ctx, cn_sd, hint, strength))
    print("controlled output rel-L2 %.2e" % err)
    assert err < UNET_TOL, err
    s.chain.set_context(ctx)
    plain = s.chain.forward(x.to(DEV), sigma.to(DEV)).cpu()
    assert rel_l2(out, plain) > 10 * UNET_TOL, rel_l2(out, plain)


# ------------------------------------------------------------------ completeness

def test_control_chain_reads_every_parameter_and_no_other():
    from controlnet_chain import ControlChain
    name = "tiny_1_7x9"
    cfg = U.config("tiny")
    c = ControlChain(cfg, DEV)
    x, sigma, ctx, hint = inputs(name)
    c.set_hint(hint)
    c.set_context(ctx)
    res = c.forward(x, sigma)
    shapes = W.controlnet_param_shapes(cfg)
    assert c.read == set(shapes), (sorted(set(shapes) - c.read), sorted(c.read - set(shapes)))
    assert [tuple(r.shape[1:]) for r in res][:4] == [(7, 9, 64)] * 3 + [(4, 5, 64)]
    assert tuple(res[-1].shape[1:3]) == (1, 2) and len(res) == len([k for k in shapes if k.startswith("zero_convs.") and k.endswith(".weight")]) + 1


def test_two_residuals_of_equal_shape_swapped_are_seen(side):
    name = "tiny_2_8x12"
    s = side("tiny")
    want, _ = s.chain_run(name)
    got = s.executor_run(name)
    H.bits_held(got, want, name)
    x, sigma, ctx, _ = inputs(name)
    res = list(want[1:-1])
    i, j = 1, 2
    assert res[i].shape == res[j].shape and not torch.equal(res[i], res[j])
    res[i], res[j] = res[j], res[i]
    s.chain.set_context(ctx)
    swapped = s.chain.forward(x, sigma, control=(res, res[0].shape[0], CASES[name][6]))
    assert not torch.equal(swapped, got[-1]), "the controlled output does not depend on which of two equal-shaped skip tensors a residual joins"
    # ... which the per-tensor rel-L2 of tests/test_controlnet_gpu.py cannot see on the residuals themselves: the set of tensors is the same
    assert sorted(float(r.float().norm()) for r in res) == sorted(float(r.float().norm()) for r in want[1:-1])
