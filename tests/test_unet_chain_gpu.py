"""The UNet executor (csrc/unet.hip) against a chain of operator calls (tests/unet_chain.py), per launch and per bit; every stage of the chain
element-wise against fp64 on the operands the network really feeds it.

B1  same launches: the chain's launch list (ops.last_launches() of every call) equals the executor's launch table (profile_launches), entry by
    entry; a mismatch names the first differing layer.
B2  same bits: torch.equal(executor, chain) for every case — also with every other case run in between on the same handle (shape history
    A, B, A: arena reuse, the plan cache, derived weights), and under the hipGraph the model_function_wrapper hook replays.  No tolerance.
    Layers held under an exception instead (a seam call reproducing the launch, held to B3's element bound): none.
B3  every stage element-wise: for each tap the fp64 reference of that one stage from the stage's own fp16 inputs, the bound of tests/errbound.py
    for its route and EB.check with the signed-bias statistic, as tests/test_routes_gpu.py / test_norm_gpu.py / test_small_kernels_gpu.py hold
    the same kernels on randn.  The operands here are post-SiLU tensors, GroupNorm statistics handed over as a producer's partials, a
    residual stream that grows block by block, real score rows and GEGLU gates.  The bias statistic of an output of fewer than 10^4 elements
    (the time embedding's one to three rows, the 2 x 2 level) gets its chance level EB.rtn_noise on top of BIAS_TOL, as the small-kernel tests
    add it; from 10^4 elements on (every shape of test_routes_gpu.py) that level is inside BIAS_TOL's own room and nothing is added.
    With LD_WRITE_PARITY=1 the worst error / bound and signed bias per stage kind and case go to profiles/unet_chain_parity.json (a record).
B4  the chain is the reference's network: its output on the unet_tiny goldens meets the golden bound of test_models_gpu.py, and one case the
    oracle's apply_model on the same inputs.
"""
import json

import pytest
import torch

import chain_harness as H
import errbound as EB
from conftest import load_golden, rel_l2
from lightdiffusion_amd import weights as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
UNET_TOL = 5e-3          # the golden bound of tests/test_models_gpu.py

# name -> (config, n or nb, (h, w), tokens, mode)
CASES = {
    "tiny_2_8x12": ("tiny", 2, (8, 12), 77, "forward"),                 # non-square, every block
    "tiny_1_7x9": ("tiny", 1, (7, 9), 77, "forward"),                   # ragged stride 2, non-2x up-resize, token counts off 8
    "tiny_3_13x4": ("tiny", 3, (13, 4), 154, "forward"),                # odd batch, two prompt chunks
    "tiny_pair1_8x8": ("tiny", 1, (8, 8), 77, "pair"),                  # pair split, dup_off, in_mod
    "tiny_pair2_8x8": ("tiny", 2, (8, 8), 77, "pair"),
    "tiny_2_8x8_eps": ("tiny", 2, (8, 8), 77, "eps"),                   # mode 2 of the output convolution
    "sd15_pair1_16x16": ("sd15", 1, (16, 16), 77, "pair"),              # row-resident conv8 levels, folded skip, W8 copies
    "sd15_4_16x16": ("sd15", 4, (16, 16), 77, "forward"),               # folded up-conv route, split-K with partials
}
SIGMAS = [2.5, 0.7, 7.0, 0.2]


def config(tag):
    return W.tiny_unet_config() if tag == "tiny" else W.sd15_unet_config()


def inputs(name):
    tag, nb, (h, w), tokens, mode = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    n_all = 2 * nb if mode == "pair" else nb
    x = (torch.randn(nb, 4, h, w, generator=g) * 3.0).to(DEV)
    sigma = torch.tensor(SIGMAS[:nb], dtype=torch.float32, device=DEV)
    ctx = torch.randn(n_all, tokens, config(tag)["context_dim"], generator=g).to(DEV)
    return x, sigma, ctx


class Side:
    """One config and weight source: the executor's handle, the chain, and per case the chain's output and taps (computed once, never changed).
    source: a WeightSource for both (None: the synthetic checkpoint); cases / inputs_of: another case table and its inputs (None: CASES / inputs).
    one_case_taps: keep the taps of ONE case at a time (a full-width case's are gigabytes): asking for another case's taps drops them and
    runs that case's chain again, which must return the bits it returned before; every case's output stays (`chain_out`)."""

    def __init__(self, tag, source=None, cases=None, inputs_of=None, one_case_taps=False):
        from lightdiffusion_amd.unet import MI355XUNet, synthetic_unet
        from unet_chain import UNetChain
        self.tag, self.cfg = tag, config(tag)
        self.cases, self.inputs = CASES if cases is None else cases, inputs if inputs_of is None else inputs_of
        mine = [c for c in self.cases.values() if c[0] == tag]
        kw = dict(max_batch=max((2 if c[4] == "pair" else 1) * c[1] for c in mine), max_hw=(max(c[2][0] for c in mine), max(c[2][1] for c in mine)),
                  max_tokens=max(c[3] for c in mine))
        self.unet = synthetic_unet(self.cfg, **kw) if source is None else MI355XUNet(self.cfg, source, **kw)
        self.chain = UNetChain(self.cfg, DEV, source=source)
        self.one_case_taps = one_case_taps
        self._chain_runs = {}

    def chain_run(self, name):
        if name not in self._chain_runs or self._chain_runs[name][1] is None:
            _, _, _, _, mode = self.cases[name]
            if self.one_case_taps:
                self._chain_runs = {k: (o, None) for k, (o, _) in self._chain_runs.items()}
                self.chain.taps = []
            x, sigma, ctx = self.inputs(name)
            self.chain.set_context(ctx)
            out = self.chain.forward(x, sigma, eps_only=mode == "eps", pair=mode == "pair")
            if name in self._chain_runs:
                H.bits_held(out, self._chain_runs[name][0], f"{name}: the chain, run again for its taps,")
            self._chain_runs[name] = (out, self.chain.taps)
        return self._chain_runs[name]

    def chain_out(self, name):
        """The chain's output of the case alone (no taps asked for: none evicted)."""
        return self._chain_runs[name][0] if name in self._chain_runs else self.chain_run(name)[0]

    def executor_run(self, name):
        _, _, _, _, mode = self.cases[name]
        x, sigma, ctx = self.inputs(name)
        self.unet.set_context(ctx)
        if mode == "pair":
            return self.unet.forward_pair(x, sigma)
        return self.unet.forward(x, sigma, eps_only=mode == "eps")

    def executor_table(self, name):
        _, _, _, _, mode = self.cases[name]
        x, sigma, ctx = self.inputs(name)
        self.unet.set_context(ctx)
        (self.unet.profile_pair if mode == "pair" else self.unet.profile)(x, sigma)
        return [r[4] for r in self.unet.profile_launches()]


side = H.side_fixture(Side)


# ------------------------------------------------------------------ B1

@pytest.mark.parametrize("name", list(CASES))
def test_same_launches(side, name):
    s = side(CASES[name][0])
    _, taps = s.chain_run(name)
    mine = H.same_launches(name, taps, s.executor_table(name))
    # what the case is in the table for (REACHES): a retuned threshold that moves it off that route must bring another shape
    names = {k for _, k in mine}
    layers = [t["name"] for t in taps]
    for want in REACHES[name]:
        assert any(k.startswith(want) for k in names) or any(l.endswith(want) for l in layers), f"{name} no longer reaches {want}: {sorted(names)}"


# kernel names (prefixes) and layer-name suffixes every case must still reach.  gn_apply_kernel on its own: a GroupNorm that ran on a
# producer's partial statistics; splitk_reduce_gn_kernel: a split over K whose second pass wrote them
_ALWAYS = ("gn_apply_kernel", "gn_stats_kernel+gn_apply_kernel", "gemm", "flash_attn2_kernel", "timestep_embed_kernel", "small_conv_in_kernel",
           "small_conv_out_kernel", "+skip")
REACHES = {
    "tiny_2_8x12": _ALWAYS + ("gemm3_kernel<64,128,conv>+splitk_reduce_gn_kernel",),
    "tiny_1_7x9": _ALWAYS,
    "tiny_3_13x4": _ALWAYS,
    "tiny_pair1_8x8": _ALWAYS + ("dup_halves_kernel",),
    "tiny_pair2_8x8": _ALWAYS + ("dup_halves_kernel",),
    "tiny_2_8x8_eps": _ALWAYS,
    # the row-resident kernel at both of its levels and behind a nearest-2x resize, the skip as a launch of its own in front of it and folded elsewhere
    "sd15_pair1_16x16": _ALWAYS + ("dup_halves_kernel", "conv8_kernel<W16>", "conv8_kernel<W16,up>", "conv8_kernel<W8,up>", ".skip_connection"),
    "sd15_4_16x16": _ALWAYS + ("upconv_kernel<256,320>+upconv_reduce_kernel", "gemm3_kernel<64,160,conv,deep>+splitk_reduce_gn_kernel"),
}


# ------------------------------------------------------------------ B2

@pytest.mark.parametrize("name", list(CASES))
def test_same_bits(side, name):
    tag, nb, (h, w), tokens, mode = CASES[name]
    s = side(tag)
    want, _ = s.chain_run(name)
    H.same_bits(name, want, s.executor_run, [o for o in CASES if o != name and CASES[o][0] == tag])
    if mode == "eps":
        return                                             # (the wrapper's contract returns the denoised latent: no eps route behind it)
    # the captured graph the model_function_wrapper hook replays (LD.py:2558-2567), first contact and a replay
    x, sigma, ctx = inputs(name)
    if mode == "pair":
        x, sigma = torch.cat([x, x]).contiguous(), torch.cat([sigma, sigma]).contiguous()
    params = {"input": x, "timestep": sigma, "c": {"c_crossattn": ctx, "transformer_options": {}}, "cond_or_uncond": [1, 0] if mode == "pair" else [0]}
    s.unet._hook.clear()
    for lap in (0, 1):
        got = s.unet(None, params)
        run = s.unet._hook[(x.shape[0], h, w)]
        assert (run.pair if mode == "pair" else run.plain).graph is not None
        H.bits_held(got, want, f"{name} under the replayed graph, lap {lap}")
    s.unet._hook.clear()


# ------------------------------------------------------------------ B3

def _stage(tap, chain, what):
    """[(error / bound, signed bias)] of one tap's output(s) against the fp64 reference of that stage."""
    import test_routes_gpu as R
    kind, i, p, out = tap["kind"], tap["inp"], tap["par"], tap["out"]
    if kind == "timestep":
        t, margin, emb, bound = EB.timestep_ref(i["sigma"], chain.log_sigmas, p["dim"], p["n"], p["sigma_mod"])
        assert float(margin.min()) > 1e-4, f"{what}: an ill-posed sigma (margin {float(margin.min()):.2e})"
        return [H.held(out, emb, bound, what, keep=torch.ones_like(emb, dtype=torch.bool))]
    if kind == "linear":
        ref, bound = EB.linear_ref(i["x"], p["w"], p["b"], None, 1.0, p["act"])
        return [H.held(out, ref, bound, what)]
    if kind == "conv_in":
        ref, bound = EB.small_conv_in_ref(i["x"], p["w"], p["b"], scale_sigma=i["sigma"])
        nb = i["x"].shape[0]
        assert torch.equal(out[nb:], out[:nb].repeat(out.shape[0] // nb - 1, 1, 1, 1)), f"{what}: the pair's second copy differs"
        return [H.held(out[:nb].reshape(ref.shape), ref, bound, what)]
    if kind == "conv_out":
        ref, bound = EB.small_conv_out_ref(i["x"], p["w"], p["b"], p["mode"], i["x_in"], i["sigma"], p["in_mod"])
        return [H.held(out, ref, bound, what)]
    if kind == "groupnorm":
        x = i["x"]
        ref, bound = EB.groupnorm_ref(x, None, p["gamma"], p["beta"], p["eps"], p["silu"])
        return [H.held(out.reshape(ref.shape), ref, bound, what)]
    if kind == "conv":
        x = i["x"]
        ref, bound, (ho, wo) = EB.conv_ref(x, p["w"], p["b"], i.get("residual"), i.get("stride", 1), None, i.get("x2"), None)
        cout = p["w"].shape[0]
        if tap.get("part") is not None:
            H.partials_held(tap["part"], out, what)
        return [H.held(out.reshape(-1, cout), ref, bound, what, image_rows=ho * wo, width=wo)]
    if kind == "upconv":
        x, (hv, wv) = i["x"], i["out_hw"]
        cout = p["w"].shape[0]
        if tap["kernel"].startswith("upconv_kernel"):
            from test_upconv_fold_gpu import fold_ref
            ref, bound = fold_ref(x, p["w"], p["b"])
            ref, bound = ref.reshape(-1, cout), bound.reshape(-1, cout)
        else:
            ref, bound, _ = EB.conv_ref(x, p["w"], p["b"], None, 1, (hv, wv))
        return [H.held(out.reshape(-1, cout), ref, bound, what, image_rows=hv * wv, width=wv)]
    if kind == "gn_conv":
        x = i["x"]
        skip = (i["s1"], i["s2"], p["wskip"], p["bskip"]) if "wskip" in p else None
        ref, bound = EB.gn_silu_conv_ref(x, p["gamma"], p["beta"], p["eps"], p["w"], p["b"], x2=i.get("x2"), rowvec=i.get("rowvec"),
                                         residual=i.get("residual"), skip=skip)
        cout = p["w"].shape[0]
        if tap.get("part") is not None:
            H.partials_held(tap["part"], out, what)
        return [H.held(out.reshape(-1, cout), ref, bound, what, image_rows=x.shape[1] * x.shape[2], width=x.shape[2])]
    if kind == "linear_ln":
        t, y = out
        tref, tb = EB.linear_ref(i["x"], p["w_prod"], p["b_prod"], i["residual"])
        a = H.held(t, tref, tb, what + " producer")
        ref, bound = R._ln_ref(i["x"], p["w_prod"], p["b_prod"], p["gamma"], p["beta"], p["w"], p["b"], t, 1e-5, p["geglu"])
        return [a, H.held(y, ref, bound, what + " consumer", bias_extra=EB.GELU_FIT_BIAS if p["geglu"] else 0.0)]
    if kind == "attention":
        q, k, v, heads = i["q"], i["k"], i["v"], chain.heads
        if 8 * q.shape[0] * heads * q.shape[1] * k.shape[1] <= 1 << 31:
            ref, bound = EB.attention_ref(q.contiguous(), k.contiguous(), v.contiguous(), heads)
        else:                                              # the same reference head by head (the heads' columns are independent): fp64 score matrices of 2 GB at the most
            d = q.shape[-1] // heads
            per = [EB.attention_ref(*(t[..., j * d:(j + 1) * d].contiguous() for t in (q, k, v)), 1) for j in range(heads)]
            ref, bound = torch.cat([r for r, _ in per], -1), torch.cat([b for _, b in per], -1)
        return [H.held(out, ref, bound, what)]
    if kind == "dup":
        for full, half in zip(out, (i["t"], i["q2"], i["x"])):
            n = half.shape[0] if half.dim() == 4 else full.shape[0] // 2
            f2 = full.reshape(2, -1)
            assert torch.equal(f2[0], half.reshape(-1)) and torch.equal(f2[1], half.reshape(-1)), f"{what}: the halves are not the shared tensor"
        return [(0.0, 0.0)]
    raise AssertionError(f"no reference for stage kind {kind}")


@pytest.mark.parametrize("name", list(CASES))
def test_every_stage_elementwise(side, name):
    s = side(CASES[name][0])
    _, taps = s.chain_run(name)
    rec, fails = H.every_stage(name, taps, lambda tap, what: _stage(tap, s.chain, what))
    print(f"PARITY {name}: " + json.dumps(rec))
    H.record("unet_chain_parity.json", name, rec)
    H.stages_held(fails, taps)


# ------------------------------------------------------------------ B4

@pytest.mark.parametrize("golden", ["unet_tiny_16x16", "unet_tiny_8x12"])
def test_chain_meets_the_golden(side, golden):
    s = side("tiny")
    g = load_golden(golden)
    s.chain.set_context(g["ctx"])
    x, sg = g["x"].to(DEV), g["sigma"].to(DEV)
    eps = s.chain.forward(x, sg, eps_only=True).cpu()
    den = s.chain.forward(x, sg).cpu()
    assert rel_l2(eps, g["eps"]) < UNET_TOL and rel_l2(den, g["denoised"]) < UNET_TOL, (rel_l2(eps, g["eps"]), rel_l2(den, g["denoised"]))


def test_chain_meets_the_oracle(side):
    from oracle import sd15_ref as O
    name = "tiny_3_13x4"
    s = side("tiny")
    out, _ = s.chain_run(name)
    x, sigma, ctx = inputs(name)
    sd = W.synth_state_dict(W.unet_param_shapes(s.cfg))
    ref = O.apply_model(sd, s.cfg, O.ModelSampling(), x.cpu(), sigma.cpu(), ctx.cpu())
    assert rel_l2(out.cpu(), ref) < UNET_TOL, rel_l2(out.cpu(), ref)
    name = "tiny_pair2_8x8"
    out, _ = s.chain_run(name)
    x, sigma, ctx = inputs(name)
    ref = O.apply_model(sd, s.cfg, O.ModelSampling(), torch.cat([x, x]).cpu(), torch.cat([sigma, sigma]).cpu(), ctx.cpu())
    assert rel_l2(out.cpu(), ref) < UNET_TOL, rel_l2(out.cpu(), ref)
