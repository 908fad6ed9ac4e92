"""CPU: the conditions the adverse-statistics GPU tests (tests/test_adverse_routes_gpu.py) rest on.

  * Window: with tests/adverse.py's weight source the fp32 oracle (oracle/sd15_ref.py on fp16-rounded weights) peaks inside [2^13, 2^15] over all
    convolution / linear / normalisation outputs of the tiny cases and stays finite: 1e4 times the synthetic checkpoint's magnitudes, a factor 2
    below fp16's 65504, so no store of a correct kernel overflows.  adverse.GAIN is fixed by this test.
  * Not vacuous: on every operand profile the fp32 emulations of the kernels' arithmetic (GroupNorm with var = msq - mu^2, the ResBlock half of
    tests/test_errbound_cpu.py, the LayerNorm fold, the epilogue with its staged fp16 tile and packed adds) stay inside the bounds of
    tests/errbound.py on every element, and six planted defects are rejected at the same magnitudes.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import adverse as A
import errbound as EB
import test_errbound_cpu as TC
from lightdiffusion_amd import weights as W

CPU = "cpu"


# ------------------------------------------------------------------ the window

def _peaks(fn):
    """(peak |output| per conv / linear / norm of the oracle during fn(), fn()'s result)."""
    from oracle import sd15_ref as O
    pk = {}
    orig = (O._conv, O._lin, O._gn)

    def wrap(f):
        def g(x, sd, p, *a, **k):
            y = f(x, sd, p, *a, **k)
            pk[p] = max(pk.get(p, 0.0), float(y.abs().max()) if bool(torch.isfinite(y).all()) else float("inf"))
            return y
        return g
    O._conv, O._lin, O._gn = (wrap(f) for f in orig)
    try:
        out = fn()
    finally:
        O._conv, O._lin, O._gn = orig
    return pk, out


def _window_case(name, gain=None):
    from oracle import sd15_ref as O
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    if name.startswith("vae"):
        cfg = W.tiny_vae_config()
        if name == "vae_dec_1_5x7":
            sd = A.state_dict("vae", W.vae_decoder_param_shapes(cfg))
            z = torch.randn(1, 4, 5, 7, generator=g)
            return lambda: O.vae_decode(sd, cfg, z)
        sd = A.state_dict("vae", W.vae_encoder_param_shapes(cfg))
        px = torch.rand(2, 24, 40, 3, generator=g)
        return lambda: O.vae_encode_moments(sd, cfg, px)
    cfg = W.tiny_unet_config()
    sd = A.state_dict("unet", W.unet_param_shapes(cfg), gain=gain)
    n, h, w, sig = (2, 8, 12, (2.5, 0.7)) if name == "unet_2_8x12" else (2, 8, 8, (14.6, 0.03))
    x = torch.randn(n, 4, h, w, generator=g) * 3.0
    ctx = torch.randn(n, 77, cfg["context_dim"], generator=g)
    return lambda: O.apply_model(sd, cfg, O.ModelSampling(), x, torch.tensor(sig), ctx)


# recorded peaks with adverse.GAIN = {unet: 16, vae: 128} (the hottest stage): see each row; half the gain leaves the UNet's 8 x 12 case below 2^13
WINDOW_CASES = ["vae_dec_1_5x7",      # 2.0e4  decoder.up.2.block.1.conv2
                "vae_enc_2_3x5",      # 1.4e4  encoder.down.2.block.1.conv2
                "unet_2_8x12",        # 1.3e4  output_blocks.9.1.transformer_blocks.0.ff.net.2
                "unet_pair_8x8"]      # 2.2e4  the same layer, sigma = (14.6, 0.03)


@pytest.mark.parametrize("name", WINDOW_CASES)
def test_window(name):
    pk, out = _peaks(_window_case(name))
    top = max(pk, key=pk.get)
    print(f"WINDOW {name}: peak {pk[top]:.4g} at {top}; output max {float(out.abs().max()):.3g}")
    assert bool(torch.isfinite(out).all()) and all(math.isfinite(v) for v in pk.values())
    assert 2.0 ** 13 <= pk[top] <= 2.0 ** 15, (top, pk[top])


@pytest.mark.parametrize("name", ["unet_2_8x12", "unet_pair_8x8"])
def test_window_at_the_chain_gain(name):
    """The executor tests run the tiny UNet at twice adverse.GAIN (the executor does not store ff.net.2's output, the oracle's hottest stage:
    adverse.CHAIN_GAIN; their window is asserted on the device, on the references of what IS stored).  The condition here: the oracle's peak over
    ALL its stages, that one included, is still inside that window's upper end 2^15.5, a factor 1.4 below 65504.  Recorded: 2.6e4 (8 x 12; 8.0e3
    over the stages the executor stores), 4.3e4 (the pair; 1.9e4)."""
    pk, out = _peaks(_window_case(name, A.CHAIN_GAIN[("unet", "tiny")]))
    stored = {k: v for k, v in pk.items() if not k.endswith(".ff.net.2")}
    print(f"WINDOW {name} at the chain gain: peak {max(pk.values()):.4g}, over the stored stages {max(stored.values()):.4g}")
    assert bool(torch.isfinite(out).all())
    assert 2.0 ** 13 <= max(pk.values()) <= 2.0 ** 15.5, max(pk.values())


def test_source_leaves_the_stream_linear_convolutions_alone():
    """Only the named layers carry the gain; every factor on a whole weight tensor or row is a power of two (so rounding commutes with it)."""
    src, cfg = A.source("unet"), W.tiny_unet_config()
    for name, shape in W.unet_param_shapes(cfg).items():
        t, s = src(name, shape), W.synth_tensor(name, shape)
        if len(shape) >= 2:
            ratio = (t / s).reshape(shape[0], -1)
            assert bool((ratio == ratio[:, :1]).all())
            vals = set(ratio[:, 0].tolist())
            stream = any(k in name for k in (".out_layers.3.", ".to_out.0.", ".ff.net.2."))
            assert vals <= ({A.GAIN["unet"], A.GAIN["unet"] * A.OUTLIER_GAIN} if stream else {1.0}), (name, vals)
        elif A.is_norm(name) and name.endswith(".weight"):
            assert 2.0 ** -7 < float(t.min()) and float(t.max()) < 2.0 ** 7
    for name in ("output_blocks.2.1.conv.weight", "input_blocks.3.0.op.weight", "input_blocks.4.0.skip_connection.weight", "input_blocks.1.1.proj_out.weight"):
        assert torch.equal(src(name, (8, 8, 1, 1)), W.synth_tensor(name, (8, 8, 1, 1)))


# ------------------------------------------------------------------ GroupNorm on groups(...)

def _gn_emul(x, ga, be, eps, silu, acc16=False, clamp=True, c1=None, swap_mu=False):
    """gn_stats_kernel + gn_apply_kernel in torch fp32 (tests/test_errbound_cpu.py::_gn_fp32) with the planted defects: acc16 — the sums kept in
    fp16 (a chain over the pixels, rounded after every pixel row); clamp=False — var = msq - mu^2 not clamped at 0; swap_mu — of a two-source concat
    split at c1, the groups inside source 1 take the mean of the group at the same position inside source 2."""
    n, hw, c = x.shape
    cpg = c // 32
    xg = x.float().reshape(n, hw, 32, cpg)
    cnt = float(hw * cpg)
    if acc16:
        s1 = torch.zeros(n, 32, dtype=torch.float16)
        s2 = torch.zeros(n, 32, dtype=torch.float16)
        for p in range(hw):
            s1 = (s1.float() + xg[:, p].sum(-1)).half()
            s2 = (s2.float() + (xg[:, p] * xg[:, p]).sum(-1)).half()
        s1, s2 = s1.float(), s2.float()
    else:
        s1, s2 = xg.sum(dim=(1, 3)), (xg * xg).sum(dim=(1, 3))
    mu = s1 / cnt
    var = s2 / cnt - mu * mu
    if clamp:
        var = var.clamp_min(0.0)
    rstd = torch.rsqrt(var + eps)
    if swap_mu:
        g1 = c1 // cpg
        mu = mu.clone()
        mu[:, :min(g1, 32 - g1)] = mu[:, g1:g1 + min(g1, 32 - g1)]
    per_c = lambda t: t.repeat_interleave(cpg, dim=1).unsqueeze(1)
    sc = per_c(rstd) * ga.float()
    sh = be.float() - per_c(mu) * sc
    y = x.float() * sc + sh
    return (F.silu(y) if silu else y).half(), s2 / cnt - mu * mu


GN_CPU = [(2, 77, 64, 0, 1e-5, False), (2, 77, 192, 128, 1e-6, True), (3, 35, 128, 0, 1e-5, True)]


@pytest.mark.parametrize("n,hw,c1,c2,eps,silu", GN_CPU)
def test_groupnorm_emulation_on_stress_groups(n, hw, c1, c2, eps, silu):
    """The correct emulation is inside errbound.groupnorm_ref on groups(...) — mu / sigma = +-30, a constant group, a group dominated by one x 64
    channel — and the cancellation term is a visible share of the bound there; fp16 sums and (two sources) the other source's mean are rejected."""
    x1, x2, ga, be = A.groups(n, hw, c1, c2, 5, CPU)
    x = x1 if x2 is None else torch.cat([x1, x2], -1)
    ref, bound, share = EB.groupnorm_ref(x1, x2, ga, be, eps, silu, parts=True)
    y, _ = _gn_emul(x, ga, be, eps, silu)
    r, s = EB.check(y, ref, bound, "groupnorm emulation on groups(...)")
    cpg = (c1 + c2) // 32
    print(f"C={c1}+{c2}: error / bound {r:.3f}, bias {s:+.2e}, cancellation share in the +30 group {float(share[..., A.G_POS * cpg]. max()):.2%}")
    assert float(share[..., A.G_POS * cpg:(A.G_POS + 1) * cpg].max()) > 0.05
    with pytest.raises(AssertionError, match="element bound"):
        EB.check(_gn_emul(x, ga, be, eps, silu, acc16=True)[0], ref, bound, "statistics accumulated in fp16")
    if c2:
        with pytest.raises(AssertionError, match="element bound"):
            EB.check(_gn_emul(x, ga, be, eps, silu, c1=c1, swap_mu=True)[0], ref, bound, "mu of the other source")


def test_unclamped_variance_of_a_constant_group_is_rejected():
    """A constant group at the `mean` profile's magnitude (36.78 = half(2.75 * 13.37): a value whose square does not sum exactly in fp32, as
    44 = 2.75 * 2^4 would): msq - mu^2 in fp32 comes out at -7e-4, far below -eps, so without the clamp rsqrt returns NaN; with it the group is
    inside the bound."""
    n, hw, c, eps = 4, 77, 64, 1e-6
    x1, _, ga, be = A.groups(n, hw, c, 0, 6, CPU)
    x = (x1.float() * 13.37).half()
    ref, bound = EB.groupnorm_ref(x, None, ga, be, eps, False)
    y, raw = _gn_emul(x, ga, be, eps, False)
    EB.check(y, ref, bound, "clamped")
    bad, raw = _gn_emul(x, ga, be, eps, False, clamp=False)
    assert float(raw[:, A.G_CONST].min()) < -eps, f"the case is vacuous: raw variance of the constant group {raw[:, A.G_CONST].tolist()}"
    with pytest.raises(AssertionError, match="non-finite"):
        EB.check(bad, ref, bound, "var not clamped")


@pytest.mark.parametrize("two_sources", [False, True], ids=["one_source", "concat"])
def test_res_half_emulation_on_stress_groups(two_sources):
    """The ResBlock half (tests/test_errbound_cpu.py::_res_half_fp32) on groups(...) with rowvec and residual at the output's magnitude: inside
    errbound.gn_silu_conv_ref, whose operand error comes from groupnorm_ref's model (cancellation term included) instead of a constant."""
    n, h, w, c1, c2, cout = 2, 5, 7, 64, 32 if two_sources else 0, 64
    x1, x2, ga, be = A.groups(n, h * w, c1, c2, 7, CPU)
    x1 = x1.reshape(n, h, w, c1)
    x2 = x2.reshape(n, h, w, c2) if c2 else None
    g = torch.Generator().manual_seed(8)
    wt = (torch.randn(cout, c1 + c2, 3, 3, generator=g) / math.sqrt(9 * (c1 + c2))).half()
    b, rowvec, res = (torch.randn(cout, generator=g) * 0.5).half(), torch.randn(n, cout, generator=g).half(), torch.randn(n, h, w, cout, generator=g).half()
    ref, bound = EB.gn_silu_conv_ref(x1, ga, be, 1e-5, wt, b, x2=x2, rowvec=rowvec, residual=res)
    y = TC._res_half_fp32(x1, x2, ga, be, 1e-5, wt, b, rowvec, res, None)
    r, s = EB.check(y, ref, bound, "ResBlock half on groups(...)", image_rows=h * w, width=w)
    assert r < 1.0
    with pytest.raises(AssertionError, match="element bound"):
        EB.check(TC._res_half_fp32(x1, x2, ga, be, 1e-5, wt, b, rowvec, res, None, stats_from=(0, 1)), ref, bound, "the neighbour's statistics")


# ------------------------------------------------------------------ the epilogue: staged fp16 tile, activation, packed adds

def _epilogue_emul(x, w, b, r, act, alpha=1.0, splits=1, round_partials=False, res_first=False, ftz=False):
    """ld_op_linear in torch fp32 with the kernels' rounding points: the tile alpha acc + bias staged in fp16, the activation on the fp16 values,
    rounded once, then the residual as an fp16 add (gemm_device.h epilogue_tile).  GEGLU: gelu(gate) rounded to fp16, times the value.  Defects:
    round_partials — each of `splits` K slices rounded to fp16 before the reduce; res_first — the residual added before the activation; ftz — the
    staged tile flushed to zero below 2^-14."""
    K = x.shape[-1]
    if splits == 1:
        acc = x.float() @ w.float().t()
    else:
        step = (K + splits - 1) // splits
        parts = [x[:, k:k + step].float() @ w[:, k:k + step].float().t() for k in range(0, K, step)]
        acc = sum(p.half().float() if round_partials else p for p in parts)
    tile = (alpha * acc + (0.0 if b is None else b.float())).half().float()
    if ftz:                                    # defect: the staged tile's subnormal values flushed to zero
        tile = torch.where(tile.abs() < 2.0 ** -14, torch.zeros_like(tile), tile)
    if act == "geglu":
        n2 = tile.shape[-1] // 2
        return (tile[:, :n2] * F.gelu(tile[:, n2:]).half().float()).half()
    rr = 0.0 if r is None else r.float()
    if res_first:
        tile = tile + rr
    y = {"none": lambda t: t, "silu": F.silu, "quick_gelu": lambda t: t * torch.sigmoid(1.702 * t)}[act](tile)
    if act != "none":
        y = y.half().float()
    return (y if res_first or r is None else y + rr).half()


@pytest.mark.parametrize("act", ["none", "silu", "quick_gelu", "geglu"])
@pytest.mark.parametrize("profile", ["big", "outlier", "heavy"])
def test_epilogue_emulation_on_profiles(profile, act):
    """The correct epilogue emulation is inside errbound.linear_ref on every profile, with a randn residual at the output's magnitude and with the
    cancelling one; under `big` the activations' arguments reach past +-88 (exp saturates) without a NaN."""
    M, N, K = 130, 192, 200
    x, w, b, mag = A.linear_operands(profile, M, N, K, act, 11, CPU)
    pre = x.double() @ w.double().t() + b.double()
    if profile == "big":
        assert float(pre.abs().max()) > 88.0
    if act == "geglu":
        ref, bound = EB.linear_ref(x, w, b, None, 1.0, act)
        r, s = EB.check(_epilogue_emul(x, w, b, None, act), ref, bound, f"{profile} geglu", bias_extra=EB.GELU_FIT_BIAS)
        return
    g = torch.Generator().manual_seed(12)
    for kind, res in (("randn", (torch.randn(M, N, generator=g) * mag).half()), ("cancel", A.cancel(EB._act(pre, act)))):
        ref, bound = EB.linear_ref(x, w, b, res, 1.0, act)
        y = _epilogue_emul(x, w, b, res, act)
        assert bool(torch.isfinite(y).all())
        # the cancelling residual leaves |y_hat| = |act(pre)| / 8 while the activation's store and the add round relative to |act(pre)|: the bias
        # statistic's chance level is that of those magnitudes (EB.rtn_noise_weighted), not of |y_hat|
        extra = EB.rtn_noise_weighted(EB._act(pre, act).abs() + ref.abs(), ref) if kind == "cancel" else 0.0
        r, s = EB.check(y, ref, bound, f"{profile} {act} residual {kind}", bias_extra=extra)
        print(f"{profile} {act} residual {kind}: error / bound {r:.3f}, bias {s:+.2e}")
        if act != "none":
            with pytest.raises(AssertionError, match="element bound"):
                EB.check(_epilogue_emul(x, w, b, res, act, res_first=True), ref, bound, "residual before the activation")


def test_subnormal_staged_value_tile_needs_its_absolute_term():
    """A GEGLU whose VALUE half lands in fp16's subnormal range (value rows times 2^-16) under a gate of up to several hundred (`outlier`): the
    staged value carries 2^-25 absolute, far more than 2^-11 of itself, and the gate multiplies it.  The correct emulation is OUTSIDE the bound
    without errbound.epilogue_ref's floor max(2^-11 |pre|, 2^-25) and inside with it; a tile flushed to zero below 2^-14 (up to 2^-14 absolute) is
    still rejected with it."""
    M, N, K = 130, 192, 200
    x = A.outlier((M, K), 17, CPU)
    g = torch.Generator().manual_seed(18)
    w = torch.randn(N, K, generator=g) / math.sqrt(K)
    b = torch.randn(N, generator=g) * 0.5
    w[:N // 2] *= 2.0 ** -16
    b[:N // 2] *= 2.0 ** -16
    w, b = w.half(), b.half()
    acc, absdot = x.double() @ w.double().t(), x.double().abs() @ w.double().abs().t()
    pre_a = (acc + b.double())[:, :N // 2]
    assert float((pre_a.abs() < 2.0 ** -14).double().mean()) > 0.2 and float(pre_a.abs().max()) > 2.0 ** -24
    y = _epilogue_emul(x, w, b, None, "geglu")
    ref, without = EB.epilogue_ref(acc, absdot, K, b, None, 1.0, "geglu", staged_subnormal=False)
    with pytest.raises(AssertionError, match="element bound"):
        EB.check(y, ref, without, "no subnormal term", bias_extra=1.0)
    ref, bound = EB.epilogue_ref(acc, absdot, K, b, None, 1.0, "geglu")
    keep = ref.abs() > 2.0 ** -14                              # the bias statistic over outputs in the normal range
    r, s = EB.check(y, ref, bound, "subnormal value tile", keep=keep, bias_extra=EB.GELU_FIT_BIAS + EB.rtn_noise(EB.independent_roundings(ref, keep)))
    print(f"subnormal staged value tile: error / bound {r:.3f}, bias {s:+.2e}")
    with pytest.raises(AssertionError, match="element bound"):
        EB.check(_epilogue_emul(x, w, b, None, "geglu", ftz=True), ref, bound, "tile flushed to zero", bias_extra=1.0)


@pytest.mark.parametrize("profile", ["big", "outlier", "heavy"])
def test_rounded_splitk_partials_are_rejected(profile):
    M, N, K = 130, 192, 2584
    x, w, b, mag = A.linear_operands(profile, M, N, K, "none", 13, CPU)
    ref, bound = EB.linear_ref(x, w, b, None, 0.75, "none")
    EB.check(_epilogue_emul(x, w, b, None, "none", 0.75, splits=4), ref, bound, "fp32 partials")
    with pytest.raises(AssertionError, match="element bound"):
        EB.check(_epilogue_emul(x, w, b, None, "none", 0.75, splits=4, round_partials=True), ref, bound, "fp16 partials")


# ------------------------------------------------------------------ the LayerNorm fold

def _ln_fold_emul(t, gamma, beta, w, bias, eps, geglu, wsum_unfolded=False, clamp=True):
    """The consumer of the LayerNorm fold in torch fp32 (gemm_device.h ln_prepare / ln_apply, misc.hip ln_fold_kernel): W' = half(w gamma),
    b' = half(bias + w beta), wsum = sum of the rounded W'; per row mu and var = msq - mu^2 from fp32 sums of the stored fp16 t;
    y = (t W'^T - mu wsum) rstd + b'.  Defect: wsum from the unfolded w."""
    c = t.shape[-1]
    wf = (w.float() * gamma.float()).half().float()
    bf = (bias.float() + w.float() @ beta.float()).half().float()
    wsum = (w.float() if wsum_unfolded else wf).sum(-1)
    tf = t.float()
    mu = tf.sum(-1, keepdim=True) / c
    var = (tf * tf).sum(-1, keepdim=True) / c - mu * mu
    rstd = torch.rsqrt((var.clamp_min(0.0) if clamp else var) + eps)
    tile = ((tf @ wf.t() - mu * wsum) * rstd + bf).half().float()
    if geglu:
        n2 = tile.shape[-1] // 2
        return (tile[:, :n2] * F.gelu(tile[:, n2:]).half().float()).half()
    return tile.half()

@pytest.mark.parametrize("geglu", [False, True], ids=["plain", "geglu"])
@pytest.mark.parametrize("ratio,scale", A.LN_STATS)
def test_ln_fold_emulation_under_large_means(ratio, scale, geglu):
    """The fold's emulation on t with mu / sigma = 30 at 2^4 and 8 at 2^7 is inside test_routes_gpu._ln_ref's bound (its cancellation term
    2^-23 rstd |mu| sum|gamma w| is what holds (acc - mu wsum) there); wsum of the unfolded w is rejected."""
    import test_routes_gpu as R
    M, C, N = 96, 320, 128
    x, wp, bp, gamma, beta, w, b = A.ln_operands(M, C, N, ratio, scale, 21, CPU)
    t = (x.float() @ wp.float().t() + bp.float()).half()
    td = t.double()
    got = float((td.mean(-1) / td.std(-1, unbiased=False)).mean())
    assert abs(got / ratio - 1.0) < 0.15, got
    ref, bound = R._ln_ref(x, wp, bp, gamma, beta, w, b, t, 1e-5, geglu)
    extra = EB.GELU_FIT_BIAS if geglu else 0.0
    r, s = EB.check(_ln_fold_emul(t, gamma, beta, w, b, 1e-5, geglu), ref, bound, "LN fold emulation", bias_extra=extra)
    print(f"mu/sigma {ratio} at {scale} geglu={geglu}: error / bound {r:.3f}, bias {s:+.2e}")
    with pytest.raises(AssertionError, match="element bound"):
        EB.check(_ln_fold_emul(t, gamma, beta, w, b, 1e-5, geglu, wsum_unfolded=True), ref, bound, "wsum of the unfolded w", bias_extra=extra)
