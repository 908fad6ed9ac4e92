"""CPU: the error-bound checker (tests/errbound.py) is sharp enough to catch the errors rel-L2 hides, and the route table of
tests/test_routes_gpu.py names every contraction kernel template the sources define."""
import math
import os
import re

import pytest
import torch

import errbound as EB
from conftest import ROOT


def _case(M=300, N=192, K=256, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g).half()
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).half()
    b = (torch.randn(N, generator=g) * 0.5).half()
    r = torch.randn(M, N, generator=g).half()
    ref, bound = EB.linear_ref(x, w, b, r)
    return x, w, b, r, ref, bound


def _rtz(ref):
    """fp16 rounding toward zero: RTN, then one step toward zero wherever RTN rounded away from zero."""
    y = ref.half()
    away = (y.double().abs() > ref.abs()) & (y != 0)
    bits = y.view(torch.int16).clone()
    bits[away] -= 1                    # sign-magnitude: one less magnitude step
    return bits.view(torch.float16)


def test_accepts_round_to_nearest_result():
    *_, ref, bound = _case()
    r, s = EB.check(ref.half(), ref, bound, "RTN")
    assert r <= 1.0 and abs(s) < 1e-5


def test_rejects_one_element_off_by_one_percent():
    *_, ref, bound = _case()
    y = ref.clone()
    y[171, 77] *= 1.01
    with pytest.raises(AssertionError, match=r"element bound: 1 of .*row 171, column 77.*tile \(1, 0\)"):
        EB.check(y.half(), ref, bound, "one element", tile=(128, 160))


def test_rejects_one_column_missing_its_bias():
    x, w, b, r, ref, bound = _case()
    y = ref.clone()
    y[:, 100] -= b[100].double()
    with pytest.raises(AssertionError, match=r"element bound: .*column 100"):
        EB.check(y.half(), ref, bound, "bias column")


def test_rejects_last_ragged_tile_without_residual():
    x, w, b, r, ref, bound = _case()
    y = ref.clone()
    y[256:] -= r[256:].double()                       # M = 300, 128-row tiles: the last tile holds rows 256..299
    with pytest.raises(AssertionError, match=r"element bound: .*tile \(2, "):
        EB.check(y.half(), ref, bound, "ragged tile", tile=(128, 160))


def test_rejects_round_toward_zero_by_the_bias_statistic():
    *_, ref, bound = _case(M=512, N=320)
    y = _rtz(ref)
    s = EB.signed_bias(y, ref)
    assert s < -EB.BIAS_TOL, s
    with pytest.raises(AssertionError, match="signed bias"):
        EB.check(y, ref, bound, "RTZ")


def test_rtn_bias_statistic_is_noise():
    *_, ref, _ = _case(M=512, N=320, seed=3)
    assert abs(EB.signed_bias(ref.half(), ref)) < EB.BIAS_TOL / 10


def _simulated_attention(q, k, v, heads, rtz):
    """The flash kernels' arithmetic without the ones column: fp32 scores from the fp16-rounded q * scale * log2(e), exp2 weights, P
    converted to fp16 (round to nearest or toward zero), numerator from the fp16 P, denominator from the unrounded fp32 weights — the
    arithmetic whose rounding mode the bias statistic has to tell apart.  (The kernels' denominator has since summed the ROUNDED weights
    without the ones column too — attention.hip — which only shrinks the error this models: _simulated_lazy_attention follows them.)"""
    b, lq, c = q.shape
    d = c // heads
    c2 = (1.0 / math.sqrt(d)) * 1.4426950408889634
    qs = (q.float() * c2).half().float().reshape(b, lq, heads, d).transpose(1, 2)
    kf = k.float().reshape(b, -1, heads, d).transpose(1, 2)
    vf = v.float().reshape(b, -1, heads, d).transpose(1, 2)
    s = qs @ kf.transpose(-1, -2)
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    ph = _rtz(p.double()) if rtz else p.half()
    o = (ph.float() @ vf) / p.sum(-1, keepdim=True)
    return o.half().transpose(1, 2).reshape(b, lq, c)


@pytest.mark.parametrize("d", [64, 160])
def test_attention_bound_accepts_rtn_and_rejects_truncated_p(d):
    g = torch.Generator().manual_seed(d)
    b, heads, lq, lk = 1, 2, 128, 256
    q, k, v = (torch.randn(b, n, heads * d, generator=g).half() for n in (lq, lk, lk))
    ref, bound = EB.attention_ref(q, k, v, heads)
    EB.check(_simulated_attention(q, k, v, heads, rtz=False), ref, bound, "RTN P")
    with pytest.raises(AssertionError, match="signed bias"):
        EB.check(_simulated_attention(q, k, v, heads, rtz=True), ref, bound, "RTZ P")
    ones = torch.ones_like(v)
    assert bool((_simulated_attention(q, k, ones, heads, rtz=False).float() == 1.0).all())
    assert float(_simulated_attention(q, k, ones, heads, rtz=True).float().max()) < 1.0


def _simulated_lazy_attention(q, k, v, heads, ones, causal, defect=None):
    """The flash kernels' lazy-reference recursion in torch fp32 (attention.hip): Q * scale * log2(e) rounded to fp16 once; per 32-key
    subtile the scores relative to the reference m_ref; the first subtile sets m_ref to its maximum, a later one moves it (per row) by
    delta = its maximum where that exceeds TAU and by 0 elsewhere; a move scales O and l by alpha = 2^-delta and shifts the scores; P is
    rounded to fp16 to nearest, numerator and denominator both sum the rounded P: the denominator as the spare V column of 1.0, part of O
    (`ones`), or in a register of its own (l_run).  defect: 'o' O not rescaled, 'l' l_run not rescaled (the register only), 'shift'
    scores not shifted after a move, 'wave' every row of a 32-row wave rescaled by the wave's largest delta (scores by their own)."""
    import attn_patterns as AP
    b, lq, c = q.shape
    lk, d = k.shape[1], c // heads
    c2 = float(torch.tensor(1.0 / math.sqrt(d), dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32))
    qs = (q.float() * c2).half().float().reshape(b, lq, heads, d).transpose(1, 2)
    kf = k.float().reshape(b, lk, heads, d).transpose(1, 2)
    vf = v.float().reshape(b, lk, heads, d).transpose(1, 2)
    m = torch.zeros(b, heads, lq, 1)
    l = torch.zeros(b, heads, lq, 1)
    o = torch.zeros(b, heads, lq, d)
    rows = torch.arange(lq).view(lq, 1)
    for t in range((lk + AP.SUB - 1) // AP.SUB):
        keys = torch.arange(t * AP.SUB, min(lk, (t + 1) * AP.SUB))
        s = qs @ kf[:, :, keys].transpose(-1, -2) - m
        if causal:
            s = s.masked_fill(keys.view(1, -1) > rows, float("-inf"))
        mx = s.amax(-1, keepdim=True)
        delta = mx if t == 0 else torch.where(mx > AP.TAU, mx, torch.zeros_like(mx))
        dscale = delta
        if defect == "wave" and t > 0:
            pad = (-lq) % 32
            dw = torch.cat([delta, torch.zeros(b, heads, pad, 1)], 2).view(b, heads, -1, 32, 1).amax(3, keepdim=True)
            dscale = dw.expand(-1, -1, -1, 32, -1).reshape(b, heads, -1, 1)[:, :, :lq]
        alpha = torch.exp2(-dscale)
        m = m + delta
        if not (defect == "shift" and t > 0):
            s = s - delta
        if defect != "o":
            o = o * alpha
        if not (defect == "l" or (defect == "o" and ones)):
            l = l * alpha
        p = torch.exp2(s)
        ph = p.half().float()
        o = o + ph @ vf[:, :, keys]
        l = l + ph.sum(-1, keepdim=True)
    return (o * (1.0 / l)).half().transpose(1, 2).reshape(b, lq, c)


PEAKED_CPU_SHAPES = [(2, 2, 100, 192, False), (1, 2, 128, 128, True)]


@pytest.mark.parametrize("b,heads,lq,lk,causal", PEAKED_CPU_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("d", [8, 40, 64, 160])
@pytest.mark.parametrize("pattern", ["spike", "stairs", "descend", "offset", "onehot"])
def test_lazy_rescale_emulation_under_peaked_scores(pattern, d, b, heads, lq, lk, causal):
    """The correct emulation of the lazy-reference recursion stays inside errbound.attention_ref's element bound and bias tolerance on every
    peaked pattern of tests/attn_patterns.py, on both denominator paths; its onehot rows equal the key's v row bit for bit; spike and stairs
    move the reference after the first subtile in at least a third of the rows."""
    import attn_patterns as AP
    q, k, v, facts = AP.make(pattern, b, heads, lq, lk, d, causal, seed=d)
    ref, bound = EB.attention_ref(q, k, v, heads, causal, p_subnormal=True)
    for ones in (True, False):
        y = _simulated_lazy_attention(q, k, v, heads, ones, causal)
        r, s = EB.check(y, ref, bound, f"{pattern} d{d} ones={ones}")
        print(f"{pattern} d{d} causal={causal} ones={ones}: error / bound {r:.3f}, signed bias {s:.2e}")
        same = AP.onehot_rows_equal_v(y, v, heads, facts)
        assert same is True, f"onehot rows differ from v: {facts['onehot'][~same].tolist()}"
    late = float(facts["moves"].any(-1).double().mean())
    if pattern in ("spike", "stairs"):
        assert late >= 1.0 / 3.0, late


@pytest.mark.parametrize("b,heads,lq,lk,causal", PEAKED_CPU_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("d", [8, 40, 64, 160])
@pytest.mark.parametrize("pattern", ["spike", "stairs"])
def test_lazy_rescale_defects_are_rejected_by_the_element_bound(pattern, d, b, heads, lq, lk, causal):
    """What a wrong rescale arm would return is outside the element bound: O not rescaled, l_run not rescaled (the unrounded denominator),
    scores not shifted after a move, the wave's largest delta used for every lane's alpha."""
    import attn_patterns as AP
    q, k, v, _ = AP.make(pattern, b, heads, lq, lk, d, causal, seed=d)
    ref, bound = EB.attention_ref(q, k, v, heads, causal, p_subnormal=True)
    for defect, ones in (("o", True), ("o", False), ("l", False), ("shift", True), ("shift", False), ("wave", True), ("wave", False)):
        with pytest.raises(AssertionError, match="element bound"):
            EB.check(_simulated_lazy_attention(q, k, v, heads, ones, causal, defect), ref, bound, f"{pattern} d{d} {defect} ones={ones}")


def test_cpu_conv_reference_matches_im2col():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 7, 5, 64, generator=g).half()
    wt = (torch.randn(32, 64, 3, 3, generator=g) / 24).half()
    for stride, out_hw in ((1, None), (2, None), (1, (11, 9)), (1, (14, 10))):
        ref, _, (ho, wo) = EB.conv_ref(x, wt, stride=stride, out_hw=out_hw)
        rows = EB.boundary_rows(ref.shape[0], 16, ho * wo, wo)
        cpu = EB.cpu_rows_conv(x, wt, rows, stride, out_hw)
        assert torch.allclose(cpu, ref[rows], rtol=1e-12, atol=1e-12), (stride, out_hw)


def test_every_contraction_kernel_template_has_a_route_row():
    """A new __global__ kernel in gemm.hip, a kernel family's source (gemm3.hip, gemm5.hip, conv6.hip, gemm7.hip, conv8.hip) or attention.hip
    cannot land without a pinned row in tests/test_routes_gpu.py
    (conv8_repack_kernel is the weight-layout copy behind conv8, not a contraction: it has no route of its own)."""
    import test_routes_gpu as R
    csrc = os.path.join(ROOT, "lightdiffusion_amd", "csrc")
    names = set()
    for f in ("gemm.hip", "gemm3.hip", "gemm5.hip", "conv6.hip", "gemm7.hip", "conv8.hip", "attention.hip"):
        names.update(re.findall(r"__global__\s+(?:__launch_bounds__\([^)]*\)\s+)?void\s+(\w+_kernel)\s*\(", open(os.path.join(csrc, f)).read()))
    names.discard("conv8_repack_kernel")
    assert {"gemm3_kernel", "gemm4_kernel", "gemm5_kernel", "conv6_kernel", "gemm7_kernel", "conv8_kernel", "splitk_reduce_kernel", "splitk_reduce_gn_kernel",
            "flash_attn2_kernel", "flash_attn512_kernel"} <= names
    pinned = {n.split("<")[0] for n in R.route_names()}
    assert not names - pinned, f"kernel templates without a route row: {sorted(names - pinned)}"


def test_every_attention_route_has_a_peaked_row():
    """An attention instantiation cannot land with flat-score coverage only: every flash_attn* route of ATTN_ROUTES is also a route of
    ATTN_PEAKED, with all five patterns (the 8-wave rows, whose fp64 reference is a few GB, with spike and onehot at least)."""
    import test_routes_gpu as R
    peaked = {}
    for row in R.ATTN_PEAKED:
        if row[0] != "qkv":
            peaked.setdefault(row[7], set()).update(row[8])
    for route in sorted({row[-1] for row in R.ATTN_ROUTES}):
        assert route.startswith("flash_attn"), route
        want = {"spike", "onehot"} if route.endswith(",8>") else set(R.ALL_PATTERNS)
        assert want <= peaked.get(route, set()), f"{route}: peaked patterns {sorted(peaked.get(route, set()))}, wanted {sorted(want)}"
    assert {row[7] for row in R.ATTN_PEAKED if row[0] == "qkv"} >= {"flash_attn2_kernel<3,rowV,plain,4>", "flash_attn2_kernel<5,rowV,plain,4>",
                                                                    "flash_attn2_kernel<10,rowV,plain,4>", "flash_attn512_kernel<512,plain>"}


def test_peaked_inputs_hold_their_margins_for_every_route_row():
    """attn_patterns.make asserts its conditions on the inputs (every threshold comparison outside the rounding window, every planted row at its
    jump, onehot margins >= 40, at most one query in 8 rescaled, the offset rows' first references) while it builds: build every case of
    ATTN_PEAKED here, and hold each case's facts to what its pattern is for."""
    import attn_patterns as AP
    import test_routes_gpu as R
    built = {}                                             # (the V layouts of one shape take the same inputs: built once; the last two kept)
    for seam, b, heads, lq, lk, d, causal, route, pattern in R.ATTN_PEAKED_CASES:
        key = (pattern, b, heads, lq, lk, d, causal)
        if key not in built:
            if len(built) == 2:
                built.pop(next(iter(built)))
            built[key] = AP.make(pattern, b, heads, lq, lk, d, causal, seed=d)[3]
        facts = built[key]
        moves, pl, jumps = facts["moves"], facts["planted"], facts["jumps"]
        nsub, what = moves.shape[-1], (route, pattern, b, heads, lq, lk, d)
        if pattern in ("spike", "stairs", "onehot"):
            assert bool(moves[..., 2:].any()), what            # a move in a subtile of the second 64-key tile or later
        if pattern == "onehot":
            assert len(facts["onehot"]) >= 4 * b * heads, what
        if pattern == "descend":
            assert not bool(moves.any()) and len(pl) >= 16 * b * heads, what
        if pattern == "spike":
            # every position of a subtile (all 16 accumulator elements of both half-waves), every later subtile, the last valid key; at least
            # a third of the jump-6 keys stand 6 .. TAU above the reference and leave it where it is (another row's key can share their subtile)
            # (causal 77 x 77 has 45 later keys, two of three of them planted: 18 positions)
            npos = len(set((pl[:, 3] % AP.SUB).tolist()))
            assert npos == AP.SUB or (lk - AP.SUB < 2 * AP.SUB and 2 * npos >= AP.SUB), what
            assert set(pl[:, 4].tolist()) == set(range(1, nsub)), what
            assert causal or bool((pl[:, 3] == lk - 1).any()), what
            six = pl[jumps == 6.0]
            assert float((facts["gaps"][six[:, 0], six[:, 1], six[:, 2], six[:, 4]] < AP.TAU).double().mean()) >= 1.0 / 3.0, what
            # some lanes of a wave move while others take delta = 0: at least an eighth of the (32-query wave, later subtile) pairs are mixed
            # (at d <= 40 hardly a ROW stays flat throughout: every query sees every planted key at 1 / sqrt(d) of its score)
            pad = (-lq) % 32
            w = torch.cat([moves[..., 1:], torch.zeros(b, heads, pad, nsub - 1, dtype=torch.bool)], 2).view(b, heads, -1, 32, nsub - 1)
            real = (torch.arange(lq + pad) < lq).view(1, 1, -1, 32, 1)
            mixed = w.any(3) & ~(w | ~real).all(3)
            assert float(mixed.double().mean()) >= 1.0 / 8.0, what
        if pattern == "stairs":
            # rows whose reference moves in EVERY later full subtile, and in the ragged last one as well (Lk = 161: it holds one key, so
            # one planted row per (batch, head))
            assert int(moves[..., 1:lk // AP.SUB].all(-1).sum()) >= 4 * b * heads and int(moves[..., 1:].all(-1).sum()) >= b * heads, what


# ------------------------------------------------------------------ the references of the norm, boundary-conv and fold kernels (norm.hip, misc.hip)
import torch.nn.functional as F


def _gn_inputs(n, hw, c, seed):
    g = torch.Generator().manual_seed(seed)
    grp = torch.arange(c) // (c // 32)
    x = (torch.randn(n, hw, c, generator=g) * (0.5 + (grp % 5).float() * 0.3) + (grp.float() - 15.5) * 0.25).half()
    return x, (1.0 + 0.5 * torch.randn(c, generator=g)).half(), (0.5 * torch.randn(c, generator=g)).half()


def _gn_fp32(x, ga, be, eps, silu, steal_mean=None):
    """gn_stats_kernel + gn_apply_kernel in torch fp32: sums of x and x^2, var = msq - mu^2, y = x sc + sh.  steal_mean = g: group g is
    normalised with the mean of group g + 1 (the defect)."""
    n, hw, c = x.shape
    cpg = c // 32
    xg = x.float().reshape(n, hw, 32, cpg)
    cnt = float(hw * cpg)
    mu = xg.sum(dim=(1, 3)) / cnt
    var = ((xg * xg).sum(dim=(1, 3)) / cnt - mu * mu).clamp_min(0.0)
    rstd = torch.rsqrt(var + eps)
    if steal_mean is not None:
        mu[:, steal_mean] = mu[:, steal_mean + 1]
    per_c = lambda t: t.repeat_interleave(cpg, dim=1).unsqueeze(1)
    sc = per_c(rstd) * ga.float()
    sh = be.float() - per_c(mu) * sc
    y = x.float() * sc + sh
    return F.silu(y) if silu else y


@pytest.mark.parametrize("n,hw,c,eps,silu", [(2, 35, 96, 1e-5, True), (1, 300, 320, 1e-6, False)])
def test_groupnorm_ref_and_bound(n, hw, c, eps, silu):
    x, ga, be = _gn_inputs(n, hw, c, c)
    ref, bound = EB.groupnorm_ref(x[..., :40].contiguous(), x[..., 40:].contiguous(), ga, be, eps, silu)
    ind = F.group_norm(x.double().transpose(1, 2), 32, ga.double(), be.double(), eps).transpose(1, 2)
    ind = ind * torch.sigmoid(ind) if silu else ind
    assert float((ref - ind).abs().max()) < 1e-12
    assert EB.bias_kept_fraction(ref) >= 0.5
    y32 = _gn_fp32(x, ga, be, eps, silu)
    EB.check(y32.half(), ref, bound, "fp32 emulation, RTN")
    with pytest.raises(AssertionError, match="signed bias"):
        EB.check(_rtz(y32.double()), ref, bound, "RTZ")
    with pytest.raises(AssertionError, match="element bound"):
        EB.check(_gn_fp32(x, ga, be, eps, silu, steal_mean=7).half(), ref, bound, "group 7 with group 8's mean")
    be2 = be.clone()
    be2[c // 2] = 0
    with pytest.raises(AssertionError, match=rf"element bound: .*, {c // 2}\)"):
        EB.check(_gn_fp32(x, ga, be2, eps, silu).half(), ref, bound, "one channel without beta")
    sc, b_sc, sh, b_sh = EB.groupnorm_scale_shift_ref(x, None, ga, be, eps)
    assert float(((x.double() * sc.unsqueeze(1) + sh.unsqueeze(1)) - EB.groupnorm_ref(x, None, ga, be, eps, False)[0]).abs().max()) < 1e-12


def test_groupnorm_bound_carries_the_cancellation_term():
    """mu / sigma = 30: the fp32 emulation of var = msq - mu^2 stays inside the bound, and the cancellation term is a visible share of it
    (the bound does not hide it in a constant)."""
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(2, 77, 64, generator=g) + 30.0).half()
    ga, be = torch.ones(64).half(), torch.zeros(64).half()
    ref, bound, share = EB.groupnorm_ref(x, None, ga, be, 1e-5, False, parts=True)
    EB.check(_gn_fp32(x, ga, be, 1e-5, False).half(), ref, bound, "mu/sigma = 30")
    x0 = (torch.randn(2, 77, 64, generator=g)).half()
    _, _, share0 = EB.groupnorm_ref(x0, None, ga, be, 1e-5, False, parts=True)
    assert float(share.max()) > 20 * float(share0.max()) and float(share0.max()) < 0.01


@pytest.mark.parametrize("rows,c", [(5, 64), (130, 520)])
def test_layernorm_ref_and_bound(rows, c):
    g = torch.Generator().manual_seed(c)
    x = torch.randn(rows, c, generator=g)
    x[1::3] += 100.0
    x = x.half()
    ga, be = (1.0 + 0.5 * torch.randn(c, generator=g)).half(), (0.5 * torch.randn(c, generator=g)).half()
    ref, bound = EB.layernorm_ref(x, ga, be, 1e-5)
    assert float((ref - F.layer_norm(x.double(), (c,), ga.double(), be.double(), 1e-5)).abs().max()) < 1e-12
    assert EB.bias_kept_fraction(ref) >= 0.5
    xf = x.float()
    mu = xf.sum(-1, keepdim=True) / c
    d = xf - mu
    emu = lambda beta: d * torch.rsqrt((d * d).sum(-1, keepdim=True) / c + 1e-5) * ga.float() + beta.float()
    EB.check(emu(be).half(), ref, bound, "fp32 emulation, RTN")
    if rows * c > 10000:
        with pytest.raises(AssertionError, match="signed bias"):
            EB.check(_rtz(emu(be).double()), ref, bound, "RTZ")
    be2 = be.clone()
    be2[3] = 0
    with pytest.raises(AssertionError, match=r"element bound: .*column 3\)"):
        EB.check(emu(be2).half(), ref, bound, "one channel without beta")


@pytest.mark.parametrize("rows,cols,valid", [(7, 40, 33), (300, 2056, 2056)])
def test_softmax_ref_and_bound(rows, cols, valid):
    g = torch.Generator().manual_seed(cols)
    s = (torch.randn(rows, cols, generator=g) * 4.0).half()
    s[:, valid:] = 100.0                                                 # pad columns hold the row's maximum
    ref, bound = EB.softmax_ref(s, valid)
    assert float((ref[:, :valid] - torch.softmax(s[:, :valid].double(), -1)).abs().max()) < 1e-12 and bool((ref[:, valid:] == 0).all())
    keep = EB.top_half_per_row(ref)
    assert abs(float(keep.double().mean()) - 0.5) < 0.03
    sf = s.float()[:, :valid]
    e = torch.exp(sf - sf.amax(-1, keepdim=True))
    p = torch.zeros(rows, cols)
    p[:, :valid] = e / e.sum(-1, keepdim=True)
    EB.check(p.half(), ref, bound, "fp32 emulation, RTN", keep=keep)
    if rows * cols > 10000:
        with pytest.raises(AssertionError, match="signed bias"):
            EB.check(_rtz(p.double()), ref, bound, "RTZ", keep=keep)
    q = torch.softmax(s.float(), -1)                                     # the pad columns taken into the maximum and the sum
    with pytest.raises(AssertionError):
        EB.check(q.half(), ref, bound, "pad not ignored", keep=keep)
        assert valid < cols


def test_bias_allowances_follow_the_number_format():
    """Tied maxima are one rounding error; a row of fp16-subnormal probabilities voids the bias statistic, a row in the normal range does not."""
    tied = torch.zeros(300, 64, dtype=torch.float64)
    tied[:, :3] = 1.0 / 3.0
    keep = EB.top_half_per_row(tied)
    assert abs(EB.independent_roundings(tied, keep) - 1.0) < 1e-9 and EB.subnormal_bias_allowance(tied, keep) == 0.0
    s = EB.signed_bias(tied.half(), tied, keep=keep)                  # half(1/3) lies 2.4e-4 below 1/3 in every row: no kernel's doing
    assert abs(s) > EB.BIAS_TOL and abs(s) < EB.BIAS_TOL + EB.rtn_noise(1)
    g = torch.Generator().manual_seed(2)
    p = torch.softmax(torch.randn(4, 4096, generator=g, dtype=torch.float64) * 4.0, -1)
    keep = EB.top_half_per_row(p)
    assert EB.subnormal_bias_allowance(p, keep) > abs(EB.signed_bias(p.half(), p, keep=keep)) > 0
    p = torch.softmax(torch.randn(300, 40, generator=g, dtype=torch.float64), -1)
    assert EB.subnormal_bias_allowance(p, EB.top_half_per_row(p)) == 0.0 and EB.independent_roundings(p) > 3000


def _oihw(w, cin):
    return EB.tapmajor_to_oihw(w, cin)


@pytest.mark.parametrize("n,cin,h,w,cout,variant", [(2, 3, 5, 7, 8, "pre"), (2, 4, 48, 48, 64, "sigma"), (1, 1, 9, 1, 8, "plain")])
def test_small_conv_in_ref_and_bound(n, cin, h, w, cout, variant):
    g = torch.Generator().manual_seed(cin + h)
    x = torch.randn(n, cin, h, w, generator=g)
    wt, b = (torch.randn(cout, 9 * cin, generator=g) / math.sqrt(9 * cin)).half(), torch.randn(cout, generator=g).half()
    sig = torch.tensor([0.03, 14.6])[:n] if variant == "sigma" else None
    pw, pb = ((torch.randn(cin, cin, generator=g) * 0.7).half(), (torch.randn(cin, generator=g) * 0.5).half()) if variant == "pre" else (None, None)
    ref, bound = EB.small_conv_in_ref(x, wt, b, sig, pw, pb)
    # independent: F.conv2d on the NCHW view of the same mirrored input
    v = x.half() if sig is None else (x * (1.0 / torch.sqrt(sig * sig + 1.0)).reshape(n, 1, 1, 1)).half()
    if pw is not None:
        v = F.conv2d(v.double(), pw.double().reshape(cin, cin, 1, 1), pb.double()).half()
    conv = lambda t, wgt, bias: F.conv2d(t, wgt, bias, padding=1).permute(0, 2, 3, 1).reshape(-1, cout)
    assert float((ref - conv(v.double(), _oihw(wt, cin).double(), b.double())).abs().max()) < 1e-12
    assert EB.bias_kept_fraction(ref) >= 0.5
    y32 = conv(v.float(), _oihw(wt, cin).float(), b.float())
    EB.check(y32.half(), ref, bound, "fp32 emulation, RTN", image_rows=h * w, width=w)
    if ref.numel() > 10000:
        with pytest.raises(AssertionError, match="signed bias"):
            EB.check(_rtz(y32.double()), ref, bound, "RTZ")
    if h > 1 and w > 1:                                                  # image 0's last pixel without its (ky, kx) = (0, 0) tap
        corner = y32.clone()
        corner[h * w - 1] -= _oihw(wt, cin).float()[:, :, 0, 0] @ v.float()[0, :, h - 2, w - 2]
        with pytest.raises(AssertionError, match=rf"element bound: .*image 0, row {h - 1}, column {w - 1}"):
            EB.check(corner.half(), ref, bound, "missing tap", image_rows=h * w, width=w)
    nob = y32.clone()
    nob[:, 5] -= b.float()[5]
    with pytest.raises(AssertionError, match=r"element bound: .*channel 5"):
        EB.check(nob.half(), ref, bound, "channel 5 without bias", image_rows=h * w, width=w)


@pytest.mark.parametrize("n,h,w,cin,cout", [(1, 5, 7, 8, 3), (2, 16, 16, 192, 4)])
def test_small_conv_out_ref_and_bound(n, h, w, cin, cout):
    g = torch.Generator().manual_seed(cin)
    x = torch.randn(n, h, w, cin, generator=g).half()
    wt = (torch.randn(cout, 9 * cin, generator=g) / math.sqrt(9 * cin)).half()
    b = torch.tensor([1.5, -1.25, 2.0, -1.75])[:cout].half()
    x_in, sigma = torch.randn(n, cout, h, w, generator=g), torch.tensor([0.03, 14.6])[:n]
    conv = lambda dt, bias: F.conv2d(x.to(dt).permute(0, 3, 1, 2), _oihw(wt, cin).to(dt), bias.to(dt), padding=1)
    v64, v32 = conv(torch.float64, b), conv(torch.float32, b)
    sg = sigma.reshape(n, 1, 1, 1)
    for mode in (0, 1, 2):
        ref, bound = EB.small_conv_out_ref(x, wt, b, mode, x_in, sigma)
        fin = lambda v: (x_in.to(v.dtype) - v.half().to(v.dtype) * sg.to(v.dtype)) if mode == 0 else \
            (((v + 1.0) * 0.5).clamp(0.0, 1.0).permute(0, 2, 3, 1).reshape(-1, cout) if mode == 1 else v)
        assert float((ref - fin(v64)).abs().max()) < 1e-12, mode
        assert EB.bias_kept_fraction(ref) >= 0.5
        EB.check(fin(v32), ref, bound, f"fp32 emulation mode {mode}")
        v_tap = v32.clone()                                              # image 0's first pixel without its centre tap
        v_tap[0, :, 0, 0] -= _oihw(wt, cin).float()[:, :, 1, 1] @ x[0, 0, 0].float()
        with pytest.raises(AssertionError, match="element bound: [1-4] of"):
            EB.check(fin(v_tap), ref, bound, "missing tap")
        with pytest.raises(AssertionError, match="element bound"):
            EB.check(fin(conv(torch.float32, b * torch.tensor([1.0, 0.0, 1.0, 1.0])[:cout]) if cout > 1 else v32 - b.float()[0]), ref, bound, "channel 1 without bias")
    ref, bound = EB.small_conv_out_ref(x, wt, b, 0, x_in, sigma)        # mode 0 with eps rounded toward zero instead of to nearest
    with pytest.raises(AssertionError, match="element bound"):
        EB.check(x_in - _rtz(v32.double()).float() * sg, ref, bound, "RTZ eps")
    ref2, _ = EB.small_conv_out_ref(torch.cat([x, x]), wt, b, 0, x_in, sigma, in_mod=n)
    assert torch.equal(ref2[:n], ref) and torch.equal(ref2[n:], ref)


def test_small_conv_out_mode0_accepts_what_mode2_accepts_near_zero():
    """Mode 0 rounds v to fp16 before x_in - eps sigma.  Near v = 0 the fp16 grid (2^-24 below 2^-14) is finer than the accumulation error
    e_v that mode 2 allows, so a device v inside e_v may round SEVERAL fp16 numbers away from the mirror's eps: a bound of one step there
    rejected a right kernel (2 to 5 outputs of a full-width UNet step).  Every v that mode 2 accepts must give an output mode 0 accepts;
    a v outside e_v by a few fp16 steps is still rejected, and away from zero the bound is the one step it was."""
    n, h, w, cin, cout = 1, 24, 24, 320, 4
    g = torch.Generator().manual_seed(7)
    x = torch.randn(n, h, w, cin, generator=g).half()
    wt = (torch.randn(cout, 9 * cin, generator=g) / math.sqrt(9 * cin)).half()
    b = torch.zeros(cout).half()
    x_in, sigma = torch.randn(n, cout, h, w, generator=g) * 3.0, torch.tensor([7.0])
    v64, e_v = EB.small_conv_out_ref(x, wt, b, 2)
    ref, bound = EB.small_conv_out_ref(x, wt, b, 0, x_in, sigma)
    ulp = EB._fp16_ulp(v64)
    fine = e_v >= 0.5 * ulp                                              # where the grid is finer than the accumulation error
    assert int(fine.sum()) >= 10 and int((~fine).sum()) >= 1000, (int(fine.sum()), int((~fine).sum()))
    out = lambda v: x_in.double() - v.half().double() * 7.0
    for sign in (1.0, -1.0):
        v_dev = v64 + sign * 0.95 * e_v
        EB.check(v_dev, v64, e_v, "mode 2 accepts")
        EB.check(out(v_dev), ref, bound, "mode 0 on the same v")
        moved = ((v_dev.half().double() - v64.half().double()).abs() / ulp)[fine]
        assert float(moved.max()) >= 2.0, "no eps moved more than one fp16 step: the case does not show the flaw"
    one_step = 7.0 * ulp + 2.0 ** -23 * (x_in.double().abs() + 2.0 * (v64.half().double() * 7.0).abs()) + 1e-30
    assert bool((bound[~fine] <= one_step[~fine]).all()), "away from zero the bound is one fp16 step at the most"
    far = v64 + 2.5 * e_v + 3.0 * ulp
    with pytest.raises(AssertionError, match="element bound"):
        EB.check(out(far), ref, bound, "v outside e_v")


def test_fold_refs_and_bounds():
    g = torch.Generator().manual_seed(12)
    for c in (64, 96):
        wpo, w2 = (torch.randn(c, c, generator=g) / math.sqrt(c)).half(), (torch.randn(c, 4 * c, generator=g) / math.sqrt(4 * c)).half()
        b2, bpo = (torch.randn(c, generator=g) * 0.3).half(), (torch.randn(c, generator=g) * 0.3).half()
        w_ref, w_b, b_ref, b_b = EB.mlp_out_fold_ref(wpo, w2, b2, bpo)
        assert float((w_ref - torch.cat([wpo.double() @ w2.double(), wpo.double()], 1)).abs().max()) < 1e-12
        assert float((b_ref - (wpo.double() @ b2.double() + bpo.double())).abs().max()) < 1e-12
        y32 = torch.cat([wpo.float() @ w2.float(), wpo.float()], 1)
        EB.check(y32.half(), w_ref, w_b, "mlp_out_fold fp32, RTN")
        EB.check((wpo.float() @ b2.float() + bpo.float()).half(), b_ref, b_b, "mlp_out_fold bias", bias_extra=EB.rtn_noise(c))
        with pytest.raises(AssertionError, match="signed bias"):
            EB.check(_rtz(y32.double()), w_ref, w_b, "RTZ")
        bad = y32.half()
        bad[3, 4 * c + 5] = (bad[3, 4 * c + 5].float() * (1 + 2.0 ** -10)).half()       # one ulp in an identity column
        with pytest.raises(AssertionError, match="element bound: 1 of"):
            EB.check(bad, w_ref, w_b, "identity column off by an ulp")
    for n, k, with_bias in ((192, 64, True), (7, 1280, False)):
        w = (torch.randn(n, k, generator=g) / math.sqrt(k)).half()
        ga, be = (1.0 + 0.5 * torch.randn(k, generator=g)).half(), (torch.randn(k, generator=g) * 0.5).half()
        b = (torch.randn(n, generator=g) * 0.3).half() if with_bias else None
        w_ref, w_b, b_ref, b_b = EB.ln_fold_ref(w, ga, be, b)
        assert float((w_ref - w.double() * ga.double()).abs().max()) < 1e-12
        assert float((b_ref - ((0 if b is None else b.double()) + w.double() @ be.double())).abs().max()) < 1e-12
        wh = (w.float() * ga.float()).half()
        EB.check(wh, w_ref, w_b, "ln_fold fp32, RTN", bias_extra=EB.rtn_noise(n * k))
        with pytest.raises(AssertionError, match="signed bias"):
            EB.check(_rtz(w_ref), w_ref, w_b, "RTZ", bias_extra=EB.rtn_noise(n * k))
        EB.check(((0 if b is None else b.float()) + w.float() @ be.float()).half(), b_ref, b_b, "ln_fold bias", bias_extra=EB.rtn_noise(n))
        s_ref, s_b = EB.wsum_ref(wh)
        EB.check(wh.float().sum(-1), s_ref, s_b, "wsum of the rounded W'", bias_extra=1.0)
        with pytest.raises(AssertionError, match="element bound"):      # wsum taken from the UNROUNDED product: what the kernel must not do
            EB.check((w.float() * ga.float()).sum(-1), s_ref, s_b, "wsum of the unrounded W'", bias_extra=1.0)


def test_pointwise_finish_and_timestep_refs():
    g = torch.Generator().manual_seed(13)
    x, wt, b = torch.randn(3, 35, 8, generator=g).half(), (torch.randn(8, 8, generator=g) * 0.4).half(), (torch.randn(8, generator=g) * 0.5).half()
    ref, bound = EB.small_pointwise_ref(x, wt, b)
    assert float((ref - F.conv1d(x.double().transpose(1, 2), wt.double().unsqueeze(-1), b.double())).abs().max()) < 1e-12
    EB.check(F.conv1d(x.float().transpose(1, 2), wt.float().unsqueeze(-1), b.float()).half().float(), ref, bound, "pointwise fp32", bias_extra=EB.rtn_noise(ref.numel()))
    t8 = (torch.randn(300, 8, generator=g) * 0.8).half()
    t8[0, :4] = torch.tensor([-1.0, 1.0, -1.25, 1.25]).half()
    ref, bound = EB.vae_out_finish_ref(t8, 3)
    assert ref[0].tolist() == [0.0, 1.0, 0.0]
    EB.check(((t8.float()[:, :3] + 1.0) * 0.5).clamp(0, 1), ref, bound, "finish fp32", keep=torch.ones_like(ref, dtype=torch.bool))
    # timestep: first-occurrence argmin and the embedding against the reference model's formula
    tab = torch.linspace(-3.5, 2.7, 257)
    tab[200] = tab[3]
    sigma = torch.tensor([float(tab[3]), float(tab[100]) + 0.007, -9.0, 9.0], dtype=torch.float64).exp().float()
    for dim in (2, 320):
        t, margin, emb, bound = EB.timestep_ref(sigma, tab, dim)
        assert t.tolist() == [3, 100, 0, 256] and float(margin.min()) > 1e-3
        half = dim // 2
        freqs = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float64) / half)
        args = t.double()[:, None] * freqs[None]
        assert float((emb - torch.cat([args.cos(), args.sin()], -1)).abs().max()) < 1e-12
        f32 = torch.exp(-9.210340371976184 * torch.arange(half, dtype=torch.float32) / half)
        a32 = t.float()[:, None] * f32[None]
        EB.check(torch.cat([a32.cos(), a32.sin()], -1).half(), emb, bound, "timestep fp32", keep=torch.ones_like(emb, dtype=torch.bool), bias_extra=EB.rtn_noise(emb.numel()))
    t6, _, emb6, _ = EB.timestep_ref(sigma[:2], tab, 8, n=6, sigma_mod=2)
    assert t6.tolist() == [3, 100] * 3


# ------------------------------------------------------------------ the references of the end convolutions, the tile blend, bislerp and the sampler helpers
def _one_ulp_off(y16, ref):
    """y16 with ONE element moved one fp16 ulp further from ref: the first element in the lower half of its binade (where U |y_hat| < 0.75 ulp, so
    the move — at least one ulp of error — is outside a bound that is the store's rounding plus a few 1e-7).  -> (perturbed copy, flat index)."""
    m, _ = torch.frexp(ref.flatten().abs())
    idx = int(torch.nonzero((m < 0.75) & (ref.flatten().abs() > 0.05))[0])
    bad = y16.clone().flatten()
    away = 1 if abs(float(bad[idx])) >= abs(float(ref.flatten()[idx])) else -1
    bits = bad.view(torch.int16)
    bits[idx] += away                                   # sign-magnitude: +1 is one step away from zero
    return bad.view(y16.shape), idx


def _end_inputs(n, h, w, cin, cout, seed, pitch=None):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, h, w, cin if pitch is None else pitch, generator=g)
    wt = (torch.randn(cout, 9 * cin, generator=g) / math.sqrt(9 * cin)).half()
    b = (torch.randn(cout, generator=g) * 0.5).half()
    return x, wt, b


def _conv32(a_nhwc, wt, b, cin):
    """The fp32 convolution of the first cin channels, [n h w][Cout]."""
    return F.conv2d(a_nhwc[..., :cin].float().permute(0, 3, 1, 2), _oihw(wt, cin).float(), b.float(), padding=1).permute(0, 2, 3, 1).reshape(-1, wt.shape[0])


@pytest.mark.parametrize("kind", ["esrgan_first", "taesd_first"])
def test_first_conv_refs_and_bounds(kind):
    n, h, w, cin = 2, 16, 16, 3 if kind == "esrgan_first" else 4
    x, wt, b = _end_inputs(n, h, w, cin, 64, cin)
    if kind == "taesd_first":
        x = x * 4.0
        x[0, 0, :4] = torch.tensor([[30.0, -30.0, 0.0, -0.0], [12.0, -12.0, 1e-3, -1e-3], [0.0] * 4, [3.0, -3.0, 9.0, -9.0]])
        ref, bound = EB.taesd_first_ref(x, wt, b)
        a64, e_a = EB.taesd_clamp_ref(x)
        assert a64[0, 0, 0].tolist() == [3.0, -3.0, 0.0, 0.0] and float(e_a[0, 0, 0].max()) == 0.0     # saturated and zero: no allowance
        big = torch.randn(200000, generator=torch.Generator().manual_seed(9)) * 3.0
        a_big, e_big = EB.taesd_clamp_ref(big)
        assert 0.0 < float((e_big > 0).double().mean()) < 0.01                                            # the flip allowance is rare
        assert float((((torch.tanh(big / 3.0) * 3.0).half().double() - a_big).abs() - e_big).max()) <= 0.0   # and fp32 tanh stays inside it
        a32 = (torch.tanh(x / 3.0) * 3.0).half()
        assert float(((a32.double() - a64).abs() - e_a).max()) <= 0.0
        ind = F.conv2d(a64.permute(0, 3, 1, 2), _oihw(wt, cin).double(), b.double(), padding=1).clamp_min(0).permute(0, 2, 3, 1).reshape(-1, 64)
        y32 = _conv32(a32, wt, b, cin).clamp_min(0)
        keep = ref > 0
    else:
        ref, bound = EB.esrgan_first_ref(x, wt, b)
        ind = F.conv2d(x.half().double().permute(0, 3, 1, 2), _oihw(wt, cin).double(), b.double(), padding=1).permute(0, 2, 3, 1).reshape(-1, 64)
        y32 = _conv32(x.half(), wt, b, cin)
        keep = None
    assert float((ref - ind).abs().max()) < 1e-12
    r, s = EB.check(y32.half(), ref, bound, "fp32 emulation, RTN", image_rows=h * w, width=w, keep=keep)
    print(f"{kind}: fp32 emulation error / bound {r:.3f}, signed bias {s:+.2e}")
    with pytest.raises(AssertionError, match="signed bias"):
        EB.check(_rtz(y32.double()), ref, bound, "RTZ", keep=keep)
    bad, idx = _one_ulp_off(y32.half(), ref)
    pix, ch = divmod(idx, 64)
    with pytest.raises(AssertionError, match=rf"element bound: 1 of .*image {pix // (h * w)}, row {pix % (h * w) // w}, column {pix % w}; channel {ch}\)"):
        EB.check(bad, ref, bound, "one ulp", image_rows=h * w, width=w, keep=keep)
    if kind == "esrgan_first":                            # the input NOT rounded to fp16 first: outside the bound
        with pytest.raises(AssertionError, match="element bound"):
            EB.check(_conv32(x, wt, b, cin).half(), ref, bound, "unrounded input")
    # image 1's first row reading image 0's last row (the border test dropped for ky = 0)
    a = (x.half() if kind == "esrgan_first" else (torch.tanh(x / 3.0) * 3.0).half()).float()
    leak = y32.clone().reshape(n, h, w, 64)
    wo = _oihw(wt, cin).float()
    leak[1, 0] += F.conv2d(a[0:1, h - 1:h].permute(0, 3, 1, 2), wo[:, :, 0:1, :], padding=(0, 1))[0, :, 0].t()
    leak = leak.clamp_min(0) if kind == "taesd_first" else leak
    with pytest.raises(AssertionError, match=r"element bound: .*image 1, row 0, column"):
        EB.check(leak.reshape(-1, 64).half(), ref, bound, "batch leak", image_rows=h * w, width=w, keep=keep)


@pytest.mark.parametrize("kind", ["esrgan_last", "taesd_last"])
def test_last_conv_refs_and_bounds(kind):
    """The two 64 -> 3 kernels write fp32: there is no store rounding for a round-toward-zero variant to bias, and one fp32 ulp is inside any bound of a
    576-long fp32 chain.  The defects here: one missing tap at one pixel, one channel without its bias, one output one fp16 ulp off; for the image, a
    rounding instead of the truncation."""
    n, h, w = 2, 9, 11
    x, wt, b = _end_inputs(n, h, w, 64, 3, 64, pitch=72)
    x = x.half()
    if kind == "taesd_last":
        b = torch.tensor([0.5, -0.25, 1.5]).half()
        ref, bound, img = EB.taesd_last_ref(x, wt, b)
        fin = lambda v: (v - 0.5) * 2.0
        assert float((ref < -1).double().mean()) > 0.05 and float((ref > 1).double().mean()) > 0.05
    else:
        ref, bound = EB.esrgan_last_ref(x, wt, b)
        fin = lambda v: v
    v64 = F.conv2d(x[..., :64].double().permute(0, 3, 1, 2), _oihw(wt, 64).double(), b.double(), padding=1).permute(0, 2, 3, 1).reshape(-1, 3)
    assert float((ref - fin(v64)).abs().max()) < 1e-12
    v32 = _conv32(x, wt, b, 64)
    keep = torch.ones_like(ref, dtype=torch.bool)
    r, s = EB.check(fin(v32), ref, bound, "fp32 emulation", image_rows=h * w, width=w, keep=keep)
    print(f"{kind}: fp32 emulation error / bound {r:.3f}, signed bias {s:+.2e}")
    tap = v32.clone()                                     # image 1's first pixel without its (ky, kx) = (2, 2) tap
    tap[h * w] -= _oihw(wt, 64).float()[:, :, 2, 2] @ x[1, 1, 1, :64].float()
    with pytest.raises(AssertionError, match=r"element bound: [1-3] of .*image 1, row 0, column 0"):
        EB.check(fin(tap), ref, bound, "missing tap", image_rows=h * w, width=w, keep=keep)
    with pytest.raises(AssertionError, match=r"element bound: .*channel 1\)"):
        EB.check(fin(_conv32(x, wt, b * torch.tensor([1.0, 0.0, 1.0]).half(), 64)), ref, bound, "channel 1 without bias", image_rows=h * w, width=w, keep=keep)
    off = fin(v32).clone()
    off[37, 2] *= 1.0 + 2.0 ** -10
    with pytest.raises(AssertionError, match=r"element bound: 1 of .*image 0, row 3, column 4; channel 2"):
        EB.check(off, ref, bound, "one fp16 ulp", image_rows=h * w, width=w, keep=keep)
    with pytest.raises(AssertionError, match="element bound"):          # the pad channels behind channel 64 read as data
        EB.check(fin(v32 + 1e-3 * x[..., 64:].float().sum(-1).reshape(-1, 1)), ref, bound, "pitch", keep=keep)
    if kind == "taesd_last":
        import numpy as np
        import usdu_ref
        d32 = fin(v32)
        u8 = torch.from_numpy(usdu_ref.to_u8(((d32 + 1.0) * 0.5).numpy())).double()
        assert float((u8 - img).abs().max()) <= 1.0 and set(u8.flatten().tolist()) >= {0.0, 255.0}
        rounded = (255.0 * ((ref + 1.0) * 0.5)).clamp(0, 255).round()   # round to nearest: half of the bytes one count up
        assert float((rounded != img).double().mean()) > 0.1


def _blend_tiles(oh, ow, c, rects, seed):
    g = torch.Generator().manual_seed(seed)
    tiles = []
    for (y0, x0, th, tw) in rects:
        ramp = lambda n: torch.minimum(torch.arange(1, n + 1), torch.arange(n, 0, -1)).float().clamp_max(4) / 4.0 * (0.5 + torch.rand(1, generator=g))
        tiles.append((torch.randn(th, tw, c, generator=g), ramp(th), ramp(tw), y0, x0))
    return tiles


def _blend32(oh, ow, c, tiles, skip=None, shift=0):
    out, div = torch.zeros(oh, ow, c), torch.zeros(oh, ow)
    for k, (ps, my, mx, y0, x0) in enumerate(tiles):
        if k == skip:
            continue
        th, tw = ps.shape[:2]
        m = my.reshape(th, 1) * (mx.roll(shift) if k == 1 else mx).reshape(1, tw)
        out[y0:y0 + th, x0:x0 + tw] += ps * m.unsqueeze(-1)
        div[y0:y0 + th, x0:x0 + tw] += m
    return out, div


def test_tile_blend_ref_and_bound():
    """fp32 accumulation in the kernel's order is inside the bound (out, div and the quotient); a feather ramp shifted by one sample in one tile, a
    tile left out, and one element 2^-20 off are outside it.  (An fp32 result has no store rounding to bias, and one fp32 ulp is inside a bound that
    counts three roundings per tile.)"""
    oh, ow, c = 40, 56, 3
    rects = [(0, 0, 24, 32), (0, 24, 24, 32), (16, 0, 24, 32), (16, 24, 24, 32), (23, 37, 17, 19), (5, 9, 17, 19)]
    tiles = _blend_tiles(oh, ow, c, rects, 1)
    out, b_out, div, b_div, quot, b_quot = EB.tile_blend_ref(oh, ow, c, tiles)
    assert float(div.min()) > 0
    o32, d32 = _blend32(oh, ow, c, tiles)
    keep = torch.ones_like(out, dtype=torch.bool)
    r = [EB.check(o32, out, b_out, "out", keep=keep)[0], EB.check(d32, div, b_div, "div", keep=keep[..., 0])[0],
         EB.check(o32 / d32.unsqueeze(-1), quot, b_quot, "quotient", keep=keep)[0]]
    print(f"tile blend fp32 emulation: error / bound {r[0]:.3f} (out), {r[1]:.3f} (div), {r[2]:.3f} (quotient)")
    for defect in (dict(shift=1), dict(skip=5)):
        o_bad, d_bad = _blend32(oh, ow, c, tiles, **defect)
        with pytest.raises(AssertionError, match="element bound"):
            EB.check(o_bad, out, b_out, str(defect), keep=keep)
        with pytest.raises(AssertionError, match="element bound"):
            EB.check(d_bad, div, b_div, str(defect), keep=keep[..., 0])
    bad = o32 / d32.unsqueeze(-1)
    bad[39, 55, 2] *= 1.0 + 2.0 ** -16
    with pytest.raises(AssertionError, match=r"element bound: 1 of .*\(39, 55, 2\)"):
        EB.check(bad, quot, b_quot, "one element", keep=keep)


def _oracle_pass(x, len_new, axis_w):
    """One pass of the oracle's bislerp in fp32 (its _slerp_rows on its _bilinear_taps), NCHW -> NCHW."""
    from oracle import sd15_ref as O
    xp = x.float().permute(0, 2, 3, 1)
    n, h, w, c = xp.shape
    if axis_w:
        lo, hi, fr = O._bilinear_taps(w, len_new)
        y = O._slerp_rows(xp[:, :, lo].reshape(-1, c), xp[:, :, hi].reshape(-1, c), fr.view(1, 1, -1, 1).expand(n, h, -1, 1).reshape(-1, 1)).view(n, h, len_new, c)
    else:
        lo, hi, fr = O._bilinear_taps(h, len_new)
        y = O._slerp_rows(xp[:, lo].reshape(-1, c), xp[:, hi].reshape(-1, c), fr.view(1, -1, 1, 1).expand(n, -1, w, 1).reshape(-1, 1)).view(n, len_new, w, c)
    return y.permute(0, 3, 1, 2).contiguous()


def test_bislerp_ref_and_bound():
    """The oracle's fp32 bislerp passes bislerp_axis_ref's bound, pass by pass, on every input of tests/test_bislerp_gpu.py (its inputs meet the
    threshold condition and its planted pairs come out at their closed-form values), and so does the recorded fixture of the reference's own run
    (tests/golden/bislerp.npz: both passes at once, so the width pass's bound is carried through the height pass with the slerp's Lipschitz constant
    away from the poles, 2 per tap, on the channel norm).  Dropping the zero-tap arm (1 / 0 instead of 0) or swapping the two taps is outside it.
    This run: worst error / bound 0.097 over the GPU test's inputs (C = 1, 6 x 5 -> 9 x 11, width pass), 0.085 for the fixture."""
    import test_bislerp_gpu as TB
    from oracle import sd15_ref as O
    everything = lambda t: torch.ones_like(t, dtype=torch.bool)
    worst = 0.0
    for case in TB.cases():
        c, h, w, hn, wn = case
        x, plants = TB.make_input(*case)
        ref1, b1, d1 = EB.bislerp_axis_ref(x, wn, True)
        t = _oracle_pass(x, wn, True)
        ref2, b2, d2 = EB.bislerp_axis_ref(t, hn, False)
        assert EB.bislerp_dots_clear_of_the_thresholds(d1) and EB.bislerp_dots_clear_of_the_thresholds(d2), case
        y = _oracle_pass(t, hn, False)
        assert torch.equal(y, O.bislerp(x, wn, hn))
        worst = max(worst, EB.check(t, ref1, b1, f"{case} width pass", keep=everything(ref1))[0], EB.check(y, ref2, b2, f"{case} height pass", keep=everything(ref2))[0])
        seen = TB.check_planted(t, x, plants, wn, True, str(case)) | TB.check_planted(y, t, plants, hn, False, str(case))
        assert seen == {k for k, *_ in plants}, case
        if c == 4 and h * w >= 30:
            assert seen == set(TB.KINDS), case
            # the defects, on the pass that holds the planted pairs
            with pytest.raises(AssertionError, match="element bound"):
                EB.check(_swapped_pass(x, wn), ref1, b1, "taps swapped", keep=everything(ref1))
            with pytest.raises(AssertionError, match="non-finite|element bound"):
                EB.check(_no_zero_arm_pass(x, wn), ref1, b1, "zero arm dropped", keep=everything(ref1))
    print(f"bislerp: the oracle's fp32 run, worst error / bound {worst:.3f}")
    assert worst < 1.0
    g = load_golden_("bislerp")
    for key, (wn, hn) in (("y2x", (12, 16)), ("y_odd", (9, 11))):
        x = g["x"]
        ref1, b1, d1 = EB.bislerp_axis_ref(x, wn, True)
        t = _oracle_pass(x, wn, True)
        EB.check(t, ref1, b1, f"fixture {key} width pass", keep=everything(ref1))
        ref2, b2, d2 = EB.bislerp_axis_ref(t, hn, False)
        assert EB.bislerp_dots_clear_of_the_thresholds(d1) and EB.bislerp_dots_clear_of_the_thresholds(d2), key
        lo, hi, _ = O._bilinear_taps(x.shape[2], hn)
        n1 = (b1 * b1).sum(1, keepdim=True).sqrt()
        carried = 2.0 * (n1[:, :, lo] + n1[:, :, hi]).expand_as(ref2)
        r, _ = EB.check(g[key], ref2, b2 + carried, f"fixture {key}", keep=everything(ref2))
        print(f"bislerp fixture {key}: error / bound {r:.3f}")


def _swapped_pass(x, len_new):
    """The width pass with r and 1 - r exchanged."""
    from oracle import sd15_ref as O
    xp = x.float().permute(0, 2, 3, 1)
    n, h, w, c = xp.shape
    lo, hi, fr = O._bilinear_taps(w, len_new)
    y = O._slerp_rows(xp[:, :, lo].reshape(-1, c), xp[:, :, hi].reshape(-1, c), (1.0 - fr).view(1, 1, -1, 1).expand(n, h, -1, 1).reshape(-1, 1))
    return y.view(n, h, len_new, c).permute(0, 3, 1, 2).contiguous()


def _no_zero_arm_pass(x, len_new):
    """The width pass normalising a zero tap by 1 / 0 (what the kernel would do without its `na > 0 ? 1 / na : 0`)."""
    from oracle import sd15_ref as O
    xp = x.float().permute(0, 2, 3, 1)
    n, h, w, c = xp.shape
    lo, hi, fr = O._bilinear_taps(w, len_new)
    a, b, r = xp[:, :, lo].reshape(-1, c), xp[:, :, hi].reshape(-1, c), fr.view(1, 1, -1, 1).expand(n, h, -1, 1).reshape(-1, 1)
    na, nb = a.norm(dim=1, keepdim=True), b.norm(dim=1, keepdim=True)
    ua, ub = a / na, b / nb
    cosw = (ua * ub).sum(1, keepdim=True)
    om = torch.acos(cosw)
    out = (torch.sin((1 - r) * om) / torch.sin(om) * ua + torch.sin(r * om) / torch.sin(om) * ub) * (na * (1 - r) + nb * r)
    out = torch.where(cosw > 1 - 1e-5, a, out)
    out = torch.where(cosw < 1e-5 - 1, a * (1 - r) + b * r, out)
    return out.view(n, h, len_new, c).permute(0, 3, 1, 2).contiguous()


def load_golden_(name):
    from conftest import load_golden
    return load_golden(name)


def test_sampler_elementwise_refs():
    """fp32 evaluation is inside cfg_combine_ref / axpby_ref in every pointer arm; a second lap that re-reads the first lap's elements, and a term
    dropped, are outside."""
    g = torch.Generator().manual_seed(21)
    den2 = torch.randn(2, 1000, generator=g) * 3.0
    everything = lambda t: torch.ones_like(t, dtype=torch.bool)
    for cfg in (0.0, 1.0, 7.5, -2.0):
        ref, bound = EB.cfg_combine_ref(den2, cfg)
        u, c = den2[0], den2[1]
        EB.check(u + (c - u) * cfg, ref[0], bound[0], f"cfg {cfg}", keep=everything(ref[0]))
        if cfg == 0.0:
            assert torch.equal(ref[0], u.double())
        else:
            with pytest.raises(AssertionError, match="element bound"):
                EB.check(torch.cat([(u + (c - u) * cfg)[:900], (u + (c - u) * cfg)[:100]]), ref[0], bound[0], "second lap repeats the first", keep=everything(ref[0]))
    x, y, z = (torch.randn(1000, generator=g) for _ in range(3))
    a, b, c = 0.7, -1.3, 2.5
    f = lambda v: float(torch.tensor(v, dtype=torch.float32))
    for yy, zz in ((y, z), (y, None), (None, z), (None, None)):
        ref, bound = EB.axpby_ref(x, f(a), yy, f(b), zz, f(c))
        v = f(a) * x
        if yy is not None:
            v = v + f(b) * yy
        if zz is not None:
            v = v + f(c) * zz
        EB.check(v, ref, bound, "axpby", keep=everything(ref))
        if zz is not None:
            with pytest.raises(AssertionError, match="element bound"):
                EB.check(v - f(c) * zz, ref, bound, "z dropped", keep=everything(ref))


KERNEL_PAT = r"__global__\s+(?:__launch_bounds__\([^)]*\)\s+)?void\s+(\w+_kernel)\s*\("
# the contraction families: held by name through the pinned routes of tests/test_routes_gpu.py
CONTRACTION_FILES = ("gemm.hip", "gemm3.hip", "gemm5.hip", "conv6.hip", "gemm7.hip", "conv8.hip", "attention.hip")
# every other translation unit with a kernel -> the test modules whose KERNELS tables hold its kernels
HOLDERS = {
    "norm.hip": ("test_norm_gpu",),
    "misc.hip": ("test_small_kernels_gpu", "test_bislerp_gpu"),
    "esrgan.hip": ("test_esrgan_conv_gpu", "test_end_convs_gpu", "test_blend_gpu"),
    "taesd.hip": ("test_taesd_conv_gpu", "test_end_convs_gpu"),
    "image.hip": ("test_usdu_gpu",),
    "lora.hip": ("test_lora_patch_gpu",),
    "clip.hip": ("test_embeddings_gpu",),
}


def test_every_norm_and_misc_kernel_is_held_by_a_gpu_test():
    """A __global__ kernel anywhere under csrc cannot land without a test that holds it element-wise or bitwise.
      * norm.hip, misc.hip, esrgan.hip, taesd.hip, image.hip, lora.hip, clip.hip: a row in the KERNELS table of one of the file's test modules
        (HOLDERS) that names tests of that module; no row for a kernel that no longer exists;
      * the contraction files: every kernel name is a prefix of a pinned route of tests/test_routes_gpu.py;
      * a source file with a kernel that is in neither list fails here.
    Exempt, each held element-wise or bitwise by the test its reason names:"""
    import importlib
    exempt = {
        "upconv_fold_kernel": "test_upconv_fold_gpu.py holds the folded weights and the route element-wise",
        "upconv_reduce_kernel": "test_upconv_fold_gpu.py (the split-K finish of the same route, held element-wise with it)",
        "skip_fold_kernel": "a copy and one fp16 add; test_conv6_skip_gpu.py holds its consumer element-wise against [w | wskip], b + bskip",
        "repack_rows_kernel": "a row permutation in front of every GEGLU route of test_routes_gpu.py, held element-wise there",
        "conv8_repack_kernel": "the weight-layout copy behind conv8, not a contraction: every conv8_kernel route of test_routes_gpu.py reads its output element-wise",
    }
    for k, why in exempt.items():
        assert re.search(r"test_\w+\.py", why) and re.search(r"element-wise|bitwise", why), (k, why)
    import test_routes_gpu as R
    csrc = os.path.join(ROOT, "lightdiffusion_amd", "csrc")
    kernels_of = lambda f: set(re.findall(KERNEL_PAT, open(os.path.join(csrc, f)).read()))
    sources = sorted(f for f in os.listdir(csrc) if f.endswith((".hip", ".h")))
    with_kernels = {f for f in sources if kernels_of(f)}
    assert with_kernels == set(HOLDERS) | set(CONTRACTION_FILES), f"source files whose kernels nobody holds: {sorted(with_kernels ^ (set(HOLDERS) | set(CONTRACTION_FILES)))}"
    held_anywhere = set()
    for f, mods in HOLDERS.items():
        names = kernels_of(f)
        tables = {}
        for m in mods:
            mod = importlib.import_module(m)
            for k, tests in mod.KERNELS.items():
                assert tests and all(callable(getattr(mod, t, None)) for t in tests), (m, k, tests)
                tables.setdefault(k, []).append(m)
        here = {k for k in tables if k in names}
        missing = names - here - set(exempt)
        assert not missing, f"{f}: kernels without an element-wise GPU test: {sorted(missing)}"
        held_anywhere |= here
    every = set().union(*(kernels_of(f) for f in HOLDERS))
    for mods in HOLDERS.values():
        for m in mods:
            gone = set(importlib.import_module(m).KERNELS) - every
            assert not gone, f"{m}: rows for kernels that no longer exist: {sorted(gone)}"
    assert not set(exempt) & held_anywhere
    pinned = {n.split("<")[0] for n in R.route_names()}
    for f in CONTRACTION_FILES:
        for k in kernels_of(f) - set(exempt):
            assert any(p.startswith(k) for p in pinned), f"{f}: {k} is on no pinned route of tests/test_routes_gpu.py"
    assert not {"bislerp_axis_kernel", "cfg_combine_kernel", "axpby_kernel"} & set(exempt)
    assert every | set().union(*(kernels_of(f) for f in CONTRACTION_FILES)) == set().union(*(kernels_of(f) for f in sources))


# ------------------------------------------------------------------ a ResBlock half on the executor's routes, and the UNet chain's module list (tests/unet_chain.py)

def _res_half_fp32(x, x2, ga, be, eps, wt, b, rowvec, residual, skip, stats_from=None, drop_rowvec=False, halve_tap=False):
    """The ResBlock half in torch fp32 with the kernels' fp16 rounding points: GroupNorm + SiLU rounded to fp16 once, fp32 convolution (+ the raw
    skip columns), the staged fp16 tile, then rowvec and residual as fp16 adds.  Defects: stats_from = (i, j): sample i is normalised with
    the statistics of sample j; drop_rowvec; halve_tap: the tap (ky, kx) = (1, 0) counts half in the image's first row (a border row's tap)."""
    xin = x if x2 is None else torch.cat([x, x2], -1)
    n, h, w, c = xin.shape
    src = xin.reshape(n, h * w, c)
    if stats_from is not None:
        i, j = stats_from
        cpg = c // 32
        g = src.float().reshape(n, h * w, 32, cpg)
        mu = g.mean(dim=(1, 3))
        var = (g * g).mean(dim=(1, 3)) - mu * mu
        mu[i], var[i] = mu[j], var[j]
        per_c = lambda t: t.repeat_interleave(cpg, dim=1).unsqueeze(1)
        y = (src.float() - per_c(mu)) * per_c(torch.rsqrt(var + eps)) * ga.float() + be.float()
        a = F.silu(y).half()
    else:
        a = _gn_fp32(src, ga, be, eps, True).half()
    a = a.reshape(n, h, w, c).permute(0, 3, 1, 2).float()
    acc = F.conv2d(a, wt.float(), None, padding=1)
    if halve_tap:
        first = F.conv2d(F.pad(a, (1, 1, 1, 1))[:, :, 1:2, :-2], wt.float()[:, :, 1:2, 0:1])      # tap (1, 0) of row 0: the pixel to the left (zero padding at column 0)
        acc[:, :, 0:1, :] -= 0.5 * first
    bias = b.float()
    if skip is not None:
        s1, s2, wsk, bsk = skip
        s = (s1 if s2 is None else torch.cat([s1, s2], -1)).permute(0, 3, 1, 2).float()
        acc = acc + F.conv2d(s, wsk.float()[:, :, None, None])
        bias = (b.float() + bsk.float()).half().float()
    y = (acc + bias.view(1, -1, 1, 1)).half()
    if rowvec is not None and not drop_rowvec:
        y = (y.float() + rowvec.float()[:, :, None, None]).half()
    if residual is not None:
        y = (y.float() + residual.permute(0, 3, 1, 2).float()).half()
    return y.permute(0, 2, 3, 1).reshape(n * h * w, -1)


@pytest.mark.parametrize("two_sources,with_skip", [(False, False), (True, False), (False, True)], ids=["in_layers", "in_layers_concat", "out_layers_skip"])
def test_gn_silu_conv_ref_and_bound(two_sources, with_skip):
    """errbound.gn_silu_conv_ref: equal to an independent fp64 evaluation; accepts the fp32 emulation under round to nearest; rejects a dropped
    row vector, the statistics of the neighbouring sample, a halved border tap, a dropped skip segment and round toward zero."""
    g = torch.Generator().manual_seed(11)
    n, h, w, c1, c2, cout = 2, 5, 7, 64, 32 if two_sources else 0, 64
    C = c1 + c2
    r = lambda *s, scale=1.0, off=0.0: (torch.randn(*s, generator=g) * scale + off).half()
    x = r(n, h, w, c1, off=0.3)
    x[1] = (x[1].float() * 1.7 - 0.8).half()                     # the two samples' statistics differ
    x2 = r(n, h, w, c2, scale=2.0, off=-0.5) if c2 else None
    ga, be = r(C, scale=0.2, off=1.0), r(C, scale=0.2)
    wt, b = r(cout, C, 3, 3, scale=1 / math.sqrt(9 * C)), r(cout, scale=0.5)
    rowvec = r(n, cout, scale=0.5)
    residual = None if with_skip else r(n, h, w, cout)
    skip = (r(n, h, w, 64, scale=2.0), None, r(cout, 64, scale=1 / math.sqrt(64)), r(cout, scale=0.5)) if with_skip else None
    ref, bound = EB.gn_silu_conv_ref(x, ga, be, 1e-5, wt, b, x2=x2, rowvec=rowvec, residual=residual, skip=skip)
    xin = (x if x2 is None else torch.cat([x, x2], -1)).double().permute(0, 3, 1, 2)
    a = F.silu(F.group_norm(xin, 32, ga.double(), be.double(), 1e-5))
    ind = F.conv2d(a, wt.double(), b.double(), padding=1) + rowvec.double()[:, :, None, None]
    if residual is not None:
        ind = ind + residual.double().permute(0, 3, 1, 2)
    if skip is not None:
        ind = ind + F.conv2d(skip[0].double().permute(0, 3, 1, 2), skip[2].double()[:, :, None, None], skip[3].double())
    assert float((ref - ind.permute(0, 2, 3, 1).reshape(-1, cout)).abs().max()) < 1e-11
    emu = lambda **kw: _res_half_fp32(x, x2, ga, be, 1e-5, wt, b, rowvec, residual, skip, **kw)
    rr, s = EB.check(emu(), ref, bound, "fp32 emulation, RTN", image_rows=h * w, width=w)
    assert rr < 1.0 and abs(s) < EB.BIAS_TOL
    with pytest.raises(AssertionError, match="element bound"):
        EB.check(emu(drop_rowvec=True), ref, bound, "row vector dropped", image_rows=h * w, width=w)
    with pytest.raises(AssertionError, match=r"element bound: .*image 0"):
        EB.check(emu(stats_from=(0, 1)), ref, bound, "sample 0 normalised with sample 1's statistics", image_rows=h * w, width=w)
    with pytest.raises(AssertionError, match=r"element bound: .*image \d, row 0"):
        EB.check(emu(halve_tap=True), ref, bound, "a border tap halved", image_rows=h * w, width=w)
    if skip is not None:
        with pytest.raises(AssertionError, match="element bound"):
            EB.check(_res_half_fp32(x, x2, ga, be, 1e-5, wt, b, rowvec, residual, (torch.zeros_like(skip[0]),) + skip[1:]), ref, bound, "skip segment dropped")
    with pytest.raises(AssertionError, match="signed bias"):
        EB.check(_rtz(ref), ref, bound, "RTZ")


@pytest.mark.parametrize("config", ["tiny", "sd15"])
def test_unet_chain_has_one_stage_per_reference_module(config):
    """The chain's module list (tests/unet_chain.py `modules`, what its forward walks) against counts derived from the config alone:
    UNetModel1.__init__ (LD.py:5379-5686) builds num_res_blocks[l] ResBlocks per level on the way down, one Downsample between levels, two in the
    middle, num_res_blocks[l] + 1 per level on the way up with one Upsample between levels; a SpatialTransformer behind each ResBlock whose
    transformer_depth entry is positive (transformer_depth_output read from its END).  Every name is a prefix of checkpoint keys, each key is owned
    by exactly one module, and the channels are those of the parameter shapes."""
    from lightdiffusion_amd import weights as W
    import unet_chain as UC
    cfg = W.tiny_unet_config() if config == "tiny" else W.sd15_unet_config()
    blocks = UC.modules(cfg)
    flat = [l for _, layers in blocks for l in layers]
    kinds = lambda k: [l for l in flat if l[0] == k]
    nrb, levels = cfg["num_res_blocks"], len(cfg["channel_mult"])
    n_in, n_out = sum(nrb), sum(r + 1 for r in nrb)
    assert len(kinds("conv_in")) == 1 and flat[0][0] == "conv_in"
    assert len(kinds("res")) == n_in + 2 + n_out
    assert len(kinds("down")) == levels - 1 and len(kinds("up")) == levels - 1
    n_st = sum(1 for d in cfg["transformer_depth"][:n_in] if d > 0) + (1 if cfg["transformer_depth_middle"] > 0 else 0) + \
        sum(1 for d in cfg["transformer_depth_output"][:n_out] if d > 0)
    assert len(kinds("st")) == n_st
    where = [b[0] for b, _ in blocks]
    assert where.count("input") == 1 + n_in + levels - 1 and where.count("middle") == 1 and where.count("output") == n_out
    # the output blocks pop the input blocks' channels in reverse: every ResBlock's cin is its in_layers norm's width, concat included
    shapes = W.unet_param_shapes(cfg)
    owned = {}
    for kind, name, cin, cout in flat:
        keys = [k for k in shapes if k.startswith(name + ".")]
        assert keys, name
        for k in keys:
            assert k not in owned, (k, name, owned.get(k))
            owned[k] = name
        if kind == "res":
            assert shapes[name + ".in_layers.0.weight"] == (cin,) and shapes[name + ".out_layers.3.weight"][0] == cout
            assert ((name + ".skip_connection.weight") in shapes) == (cin != cout)
        elif kind == "st":
            assert shapes[name + ".norm.weight"] == (cin,) and cin == cout
        else:
            assert shapes[name + ".weight"][:2] == (cout, cin)
    rest = set(shapes) - set(owned)
    assert rest == {"time_embed.0.weight", "time_embed.0.bias", "time_embed.2.weight", "time_embed.2.bias", "out.0.weight", "out.0.bias",
                    "out.2.weight", "out.2.bias"}, sorted(rest)
    # the transformers sit where the depth lists say: the last transformer_depth_output entries belong to the FIRST output blocks
    out_blocks = [layers for (w_, _), layers in blocks if w_ == "output"]
    tdo = cfg["transformer_depth_output"][:n_out]
    assert [any(l[0] == "st" for l in layers) for layers in out_blocks] == [d > 0 for d in reversed(tdo)]


# ------------------------------------------------------------------ what the VAE chain adds (tests/vae_chain.py, tests/test_vae_chain_gpu.py)

def _down_fp32(xpadded_nchw, wt, b):
    """The encoder's downsample in torch fp32 from an already padded fp16 image [n][C][H + 1][W + 1]: fp32 sums, one fp16 rounding."""
    return (F.conv2d(xpadded_nchw.float(), wt.float(), None, stride=2) + b.float().view(1, -1, 1, 1)).half().permute(0, 2, 3, 1).reshape(-1, wt.shape[0])


@pytest.mark.parametrize("hw", [(8, 6), (7, 5)], ids=["even", "odd"])
def test_asymmetric_pad_conv_reference(hw):
    """errbound.im2col / conv_ref / cpu_rows_conv with the pad (0, 1, 0, 1) of the VAE encoder's Downsample (LD.py:3514-3528): equal to fp64
    F.conv2d(F.pad(x, (0, 1, 0, 1)), w, stride=2); the fp32 emulation passes; a symmetric pad, a bottom row whose out-of-image taps read the next
    image's first row and a right column whose out-of-image taps read the next pixel row's first pixel (what a loader without a bounds check
    finds at those addresses in NHWC memory) are rejected, each at the row or column it spoils."""
    g = torch.Generator().manual_seed(23)
    n, (h, w), c, cout = 2, hw, 64, 32
    x = torch.randn(n, h, w, c, generator=g).half()
    x[1, 0] = (x[1, 0].float() * 8.0).half()                       # large values in the second image's first pixel row
    x[:, :, 0] = (x[:, :, 0].float() * 4.0).half()                 # ... and in every row's first pixel
    wt = (torch.randn(cout, c, 3, 3, generator=g) / math.sqrt(9 * c)).half()
    b = (torch.randn(cout, generator=g) * 0.5).half()
    ref, bound, (ho, wo) = EB.conv_ref(x, wt, b, stride=2, pad=EB.DOWNSAMPLE_PAD)
    assert (ho, wo) == ((h + 1 - 3) // 2 + 1, (w + 1 - 3) // 2 + 1) == EB.conv_out_hw(h, w, 3, 2, EB.DOWNSAMPLE_PAD)
    xn = x.permute(0, 3, 1, 2)
    ind = F.conv2d(F.pad(xn.double(), (0, 1, 0, 1)), wt.double(), b.double(), stride=2)
    assert float((ref - ind.permute(0, 2, 3, 1).reshape(-1, cout)).abs().max()) < 1e-11
    rows = list(range(ref.shape[0]))
    cpu = EB.cpu_rows_conv(x, wt, rows, 2, pad=EB.DOWNSAMPLE_PAD) + b.double()
    assert torch.allclose(cpu, ref, rtol=1e-12, atol=1e-12)
    where = dict(image_rows=ho * wo, width=wo)
    r, s = EB.check(_down_fp32(F.pad(xn, (0, 1, 0, 1)), wt, b), ref, bound, "fp32 emulation, RTN", **where)
    assert r < 1.0 and abs(s) < EB.BIAS_TOL + EB.rtn_noise(ref.numel())
    if h % 2 == 0:                                                  # (pad 1 all round gives the same output size at an even size only)
        sym = (F.conv2d(xn.float(), wt.float(), b.float(), stride=2, padding=1)).half().permute(0, 2, 3, 1).reshape(-1, cout)
        assert sym.shape == ref.shape
        with pytest.raises(AssertionError, match="element bound"):
            EB.check(sym, ref, bound, "pad 1 on all sides", **where)
    # the row below the image: the next image's first row (image 0 only: nothing of the test lies behind the last image)
    below = torch.zeros(n, c, 1, w, dtype=torch.float16)
    below[0] = xn[1, :, 0:1]
    spoiled = F.pad(torch.cat([xn, below], dim=2), (0, 1, 0, 0))
    if (h + 1 - 3) % 2 == 0:                                        # (the last output row reads the pad row: an even height)
        with pytest.raises(AssertionError, match=rf"element bound: .*image 0, row {ho - 1}, "):
            EB.check(_down_fp32(spoiled, wt, b), ref, bound, "bottom taps read the next image", **where)
    # the column right of the image: the first pixel of the next pixel row
    flat = torch.cat([xn.permute(0, 2, 3, 1).reshape(-1, c), torch.zeros(1, c, dtype=torch.float16)])          # NHWC memory, then one pixel of zeros
    right = flat[torch.arange(n * h * w).reshape(n, h, w)[:, :, -1] + 1].permute(0, 2, 1).unsqueeze(-1)            # [n][C][h][1]
    spoiled = F.pad(torch.cat([xn, right], dim=3), (0, 0, 0, 1))
    if (w + 1 - 3) % 2 == 0:
        with pytest.raises(AssertionError, match=rf"element bound: .*column {wo - 1}; "):
            EB.check(_down_fp32(spoiled, wt, b), ref, bound, "right taps read the next row", **where)


def test_linear_batched_reference_and_pad_columns():
    """errbound.linear_batched_ref (bias along the rows, n_valid), pad_columns_held and pv_ref: equal to an independent fp64 evaluation; the fp32
    emulation passes; a bias added along the columns instead, one batch element read at its neighbour's stride and scores over the pad keys
    (n_valid = Lp: the softmax's denominator then counts them) are rejected; P with a non-zero pad column is refused outright."""
    g = torch.Generator().manual_seed(31)
    n, C, L = 2, 64, 35
    Lp = (L + 7) // 8 * 8
    r = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).half()
    wv, bv, x = r(C, C, scale=1 / math.sqrt(C)), r(C, scale=0.5), r(n, L, C)
    # V^T = Wv x_b^T + bv: bias along the rows
    ref, bound = EB.linear_batched_ref(wv.unsqueeze(0).expand(n, C, C), x, bias_m=bv, n_valid=L)
    ind = torch.einsum("ok,blk->bol", wv.double(), x.double()) + bv.double().view(1, C, 1)
    assert ref.shape == (n, C, L) and float((ref - ind).abs().max()) < 1e-12
    emu = (torch.einsum("ok,blk->bol", wv.float(), x.float()) + bv.float().view(1, C, 1)).half()
    rr, s = EB.check(emu, ref, bound, "fp32 emulation, RTN")
    assert rr < 1.0 and abs(s) < EB.BIAS_TOL + EB.rtn_noise(ref.numel())
    with pytest.raises(AssertionError, match="element bound"):
        EB.check((torch.einsum("ok,blk->bol", wv.float(), x.float()) + bv.float()[:L].view(1, 1, L)).half(), ref, bound, "bias along the columns")
    with pytest.raises(AssertionError, match=r"element bound: .*element \(1, "):
        EB.check(torch.stack([emu[0], emu[0]]), ref, bound, "batch 1 read at batch 0's address")
    stored = torch.cat([emu, emu[..., L - 1:L].expand(n, C, Lp - L)], dim=-1)
    EB.pad_columns_held(stored, L, "V^T")
    with pytest.raises(AssertionError, match="pad columns"):
        EB.pad_columns_held(torch.cat([emu, torch.zeros(n, C, Lp - L, dtype=torch.float16)], dim=-1), L, "V^T zero-filled")
    # S = Q K^T / sqrt(C), P = softmax over the valid keys, O = P V
    q, k = r(n, L, C), r(n, L, C)
    sref, sbound = EB.linear_batched_ref(q, k, n_valid=L, alpha=1 / math.sqrt(C))
    assert float((sref - q.double() @ k.double().transpose(1, 2) / math.sqrt(C)).abs().max()) < 1e-12
    s16 = (q.float() @ k.float().transpose(1, 2) / math.sqrt(C)).half()
    EB.check(s16, sref, sbound, "scores, fp32 emulation")
    spad = torch.cat([s16, s16[..., L - 1:L].expand(n, L, Lp - L)], dim=-1)
    pref, pbound = EB.softmax_ref(spad.reshape(n * L, Lp), L)
    p16 = pref.half()
    assert bool((p16[:, L:] == 0).all())
    EB.check(p16, pref, pbound, "softmax over the valid keys", keep=EB.top_half_per_row(pref))
    with pytest.raises(AssertionError, match="element bound"):           # the pad keys' repeated scores join the denominator
        EB.check(torch.softmax(spad.float().reshape(n * L, Lp), -1).half(), pref, pbound, "softmax over all Lp keys")
    vt = stored.clone()
    vt[..., L:] = 3.0e4                                                   # whatever the pad columns of V^T hold, it is finite and meets zeros
    oref, obound = EB.pv_ref(p16.view(n, L, Lp), vt, L)
    oind = pref.view(n, L, Lp)[..., :L].half().double() @ stored.double()[..., :L].transpose(1, 2)
    assert float((oref - oind).abs().max()) < 1e-12
    EB.check((p16.view(n, L, Lp).float() @ vt.float().transpose(1, 2)).half(), oref, obound, "P V, fp32 emulation")
    bad = p16.view(n, L, Lp).clone()
    bad[1, 3, L] = 2.0 ** -20
    with pytest.raises(AssertionError, match="not exactly zero"):
        EB.pv_ref(bad, vt, L)


def _gn_from(x, stats_of, ga, be, eps, silu):
    """GroupNorm (+SiLU) of x [n][hw][C] in torch fp32 with the group statistics of ANOTHER tensor of the same shape (a handover gone wrong)."""
    n, hw, c = x.shape
    cpg = c // 32
    sg = stats_of.float().reshape(n, hw, 32, cpg)
    mu = sg.mean(dim=(1, 3))
    var = ((sg * sg).mean(dim=(1, 3)) - mu * mu).clamp_min(0.0)
    per_c = lambda t: t.repeat_interleave(cpg, dim=1).unsqueeze(1)
    y = (x.float() - per_c(mu)) * per_c(torch.rsqrt(var + eps)) * ga.float() + be.float()
    return (F.silu(y) if silu else y).half()


@pytest.mark.parametrize("silu", [False, True], ids=["norm", "norm_silu"])
def test_groupnorm_ref_rejects_handed_over_statistics_of_another_tensor(silu):
    """The statistics handover of csrc/vae.hip (VRun::st_of / wrote / gn) gone wrong, on errbound.groupnorm_ref — the stage reference of norm_out
    and, inside gn_silu_conv_ref, of every ResnetBlock half: the same arithmetic with the tensor's own statistics passes; with the statistics
    of the tensor that lay at the same address before (the same layer's output one step earlier: 2 % larger, shifted by 0.01 — a plausible
    image) or of the neighbouring sample it is rejected.  (gn_silu_conv_ref's neighbour control: test_gn_silu_conv_ref_and_bound.)"""
    x, ga, be = _gn_inputs(2, 60, 128, 41)
    x[1] = (x[1].float() * 1.3 + 0.2).half()
    ref, bound = EB.groupnorm_ref(x, None, ga, be, 1e-6, silu)
    rr, s = EB.check(_gn_from(x, x, ga, be, 1e-6, silu), ref, bound, "own statistics")
    assert rr < 1.0 and abs(s) < EB.BIAS_TOL
    prev = (x.float() * 1.02 + 0.01).half()
    with pytest.raises(AssertionError, match="element bound"):
        EB.check(_gn_from(x, prev, ga, be, 1e-6, silu), ref, bound, "statistics of the previous tensor at this address")
    with pytest.raises(AssertionError, match="element bound"):
        EB.check(_gn_from(x, x.flip(0), ga, be, 1e-6, silu), ref, bound, "statistics of the neighbouring sample")


def test_gn_silu_conv_ref_rejects_stale_statistics():
    """... and through the convolution (errbound.gn_silu_conv_ref, the ResnetBlock half's reference): a half normalised with the statistics
    of the previous tensor at the same address is rejected."""
    g = torch.Generator().manual_seed(43)
    n, h, w, c, cout = 2, 5, 7, 64, 64
    r = lambda *s, scale=1.0, off=0.0: (torch.randn(*s, generator=g) * scale + off).half()
    x = r(n, h, w, c, off=0.3)
    ga, be = r(c, scale=0.2, off=1.0), r(c, scale=0.2)
    wt, b, res = r(cout, c, 3, 3, scale=1 / math.sqrt(9 * c)), r(cout, scale=0.5), r(n, h, w, cout)
    ref, bound = EB.gn_silu_conv_ref(x, ga, be, 1e-6, wt, b, residual=res)

    def half_with(stats_of):
        a = _gn_from(x.reshape(n, h * w, c), stats_of.reshape(n, h * w, c), ga, be, 1e-6, True).reshape(n, h, w, c).permute(0, 3, 1, 2).float()
        y = (F.conv2d(a, wt.float(), None, padding=1) + b.float().view(1, -1, 1, 1)).half()
        return (y.float() + res.permute(0, 3, 1, 2).float()).half().permute(0, 2, 3, 1).reshape(n * h * w, cout)
    EB.check(half_with(x), ref, bound, "own statistics", image_rows=h * w, width=w)
    with pytest.raises(AssertionError, match="element bound"):
        EB.check(half_with((x.float() * 1.02 + 0.01).half()), ref, bound, "stale statistics", image_rows=h * w, width=w)


def _vae_cfg(tag):
    from lightdiffusion_amd import weights as W
    return {"tiny": W.tiny_vae_config(), "sd15": W.sd15_vae_config(), "fallback": dict(z_channels=4, ch=64, ch_mult=[1, 1, 1, 1], num_res_blocks=2, out_ch=3)}[tag]


@pytest.mark.parametrize("config", ["tiny", "sd15", "fallback"])
@pytest.mark.parametrize("encoder", [False, True], ids=["decoder", "encoder"])
def test_vae_chain_has_one_stage_per_reference_module(config, encoder):
    """The chain's module list (tests/vae_chain.py `modules`) against counts derived from the config alone: Decoder.__init__ (LD.py:3761-3855)
    builds num_res_blocks + 1 ResnetBlocks per level and one Upsample between levels, Encoder.__init__ (LD.py:3649-3729) num_res_blocks per
    level and one Downsample between levels; two ResnetBlocks around one AttnBlock in the middle of either; nin_shortcut exactly where
    cin != cout.  Every name is a prefix of checkpoint keys, each key is owned by exactly one module, and the channels are the parameters'."""
    from lightdiffusion_amd import weights as W
    import vae_chain as VC
    cfg = _vae_cfg(config)
    mods = VC.modules(cfg, encoder)
    kinds = lambda k: [m for m in mods if m[0] == k]
    levels, nrb = len(cfg["ch_mult"]), cfg["num_res_blocks"]
    assert mods[0][0] == "conv_in" and len(kinds("conv_in")) == 1
    assert len(kinds("res")) == levels * (nrb if encoder else nrb + 1) + 2
    assert len(kinds("attn")) == 1 and len(kinds("down" if encoder else "up")) == levels - 1 and not kinds("up" if encoder else "down")
    assert [m[0] for m in mods[-3:]] == ["norm_out", "conv_out", "quant"] if encoder else [m[0] for m in mods[-2:]] == ["norm_out", "conv_out"]
    i = [m[0] for m in mods].index("attn")
    assert mods[i - 1][0] == "res" and mods[i + 1][0] == "res" and ".mid." in mods[i][1]
    # per level: its ResnetBlocks, then the resampling (not behind the last level of the walk)
    walk = [m for m in mods if m[0] in ("res", "up", "down") and ".mid." not in m[1]]
    per = nrb if encoder else nrb + 1
    want = []
    for step in range(levels):
        want += ["res"] * per + ([] if step == levels - 1 else ["down" if encoder else "up"])
    assert [m[0] for m in walk] == want
    shapes = W.vae_encoder_param_shapes(cfg) if encoder else W.vae_decoder_param_shapes(cfg)
    owned = {}
    for kind, name, cin, cout in mods:
        keys = [k for k in shapes if k.startswith(name + ".")]
        assert keys, name
        for k in keys:
            assert k not in owned, (k, name, owned.get(k))
            owned[k] = name
        if kind == "res":
            assert shapes[name + ".norm1.weight"] == (cin,) and shapes[name + ".conv2.weight"][:2] == (cout, cout) and shapes[name + ".conv1.weight"][:2] == (cout, cin)
            assert ((name + ".nin_shortcut.weight") in shapes) == (cin != cout)
        elif kind == "attn":
            assert shapes[name + ".norm.weight"] == (cin,) and cin == cout and all(shapes[f"{name}.{t}.weight"] == (cin, cin, 1, 1) for t in ("q", "k", "v", "proj_out"))
        elif kind == "norm_out":
            assert shapes[name + ".weight"] == (cin,)
        else:
            assert shapes[name + ".weight"][:2] == (cout, cin)
    rest = set(shapes) - set(owned)
    assert rest == (set() if encoder else {"post_quant_conv.weight", "post_quant_conv.bias"}), sorted(rest)
    # the chain of channels is unbroken, and the widths are the config's
    for a, b in zip(mods, mods[1:]):
        assert a[3] == b[2], (a, b)
    mid = cfg["ch"] * cfg["ch_mult"][-1]
    assert mods[i][2] == mid and (mods[0][3] == cfg["ch"] if encoder else mods[0][3] == mid)
