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
    converted to fp16 (round to nearest or toward zero), numerator from the fp16 P, denominator from the unrounded fp32 weights."""
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
    rounded to fp16 to nearest, the numerator sums the rounded P, the denominator the rounded P (`ones`: the spare V column of 1.0, part
    of O) or the unrounded weights (l_run).  defect: 'o' O not rescaled, 'l' l_run not rescaled (the unrounded denominator only), 'shift'
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
        l = l + (ph if ones else p).sum(-1, keepdim=True)
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
    for seam, b, heads, lq, lk, d, causal, route, pattern in R.ATTN_PEAKED_CASES:
        facts = AP.make(pattern, b, heads, lq, lk, d, causal, seed=d)[3]
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


def test_every_norm_and_misc_kernel_is_held_by_a_gpu_test():
    """A __global__ kernel in norm.hip or misc.hip cannot land without a row in the KERNELS table of tests/test_norm_gpu.py or
    tests/test_small_kernels_gpu.py that names a test of that module.  Exempt, each held element-wise or bitwise elsewhere:"""
    exempt = {
        "upconv_fold_kernel": "test_upconv_fold_gpu.py holds the folded weights and the route element-wise",
        "upconv_reduce_kernel": "test_upconv_fold_gpu.py (the split-K finish of the same route)",
        "skip_fold_kernel": "a copy and one fp16 add; test_conv6_skip_gpu.py holds its consumer element-wise against [w | wskip], b + bskip",
        "repack_rows_kernel": "a row permutation in front of every GEGLU route of test_routes_gpu.py",
        "fill_half_kernel": "a constant fill",
        "cfg_combine_kernel": "fp32 elementwise, test_ops_gpu.py::test_sampler_elementwise",
        "axpby_kernel": "fp32 elementwise, test_ops_gpu.py::test_sampler_elementwise",
        "bislerp_axis_kernel": "test_configs_gpu.py::test_bislerp_on_device",
    }
    import test_norm_gpu as TN
    import test_small_kernels_gpu as TS
    csrc = os.path.join(ROOT, "lightdiffusion_amd", "csrc")
    pat = r"__global__\s+(?:__launch_bounds__\([^)]*\)\s+)?void\s+(\w+_kernel)\s*\("
    for f, mod in (("norm.hip", TN), ("misc.hip", TS)):
        names = set(re.findall(pat, open(os.path.join(csrc, f)).read()))
        assert names, f
        missing = names - set(mod.KERNELS) - set(exempt)
        assert not missing, f"{f}: kernels without an element-wise GPU test: {sorted(missing)}"
        assert not set(mod.KERNELS) - names, f"{f}: rows for kernels that no longer exist: {sorted(set(mod.KERNELS) - names)}"
        for k, tests in mod.KERNELS.items():
            assert tests and all(callable(getattr(mod, t, None)) for t in tests), (k, tests)
    assert not set(exempt) & (set(TN.KERNELS) | set(TS.KERNELS))
