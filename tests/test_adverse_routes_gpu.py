"""The pinned routes of tests/test_routes_gpu.py at real-checkpoint activation statistics (tests/adverse.py).

No shape is new: every case is an existing, already smallest row of that module's tables, run again on operands at 2^10, with outlier channels and
rows, with heavy tails, with means of 30 standard deviations, and with a residual that cancels 7/8 of the contraction.  Each case asserts the same
route string first, then EB.check on every element and the signed bias.  All bounds of tests/errbound.py scale with the operands, so a correct
kernel passes at any magnitude; tests/test_adverse_cpu.py holds that the bounds still reject the planted defects there.

The bias statistic under a cancelling residual gets its chance level EB.rtn_noise_weighted on top of BIAS_TOL: the stores round relative to
|act(pre)| = 8 |y_hat|, so the statistic's noise is eight times that of an output of the same size whose roundings are relative to |y_hat|.

test_overflow_policy holds what a store does past 65504 (common.h: "fp16 storage would have turned an overflow into inf"): an element whose every
stage stays below 65504 (1 - 2^-9) is finite and inside its bound, one with a stage above 65520 (1 + 2^-9) is +-inf with that stage's sign, and its
neighbours in the same tile row are unaffected; SiLU / quick-GELU absorb a tile at -inf into -0.

With LD_WRITE_PARITY=1 the worst error / bound and signed bias of every case go to profiles/adverse_parity.json (a record).
"""
import math

import pytest
import torch

import adverse as A
import errbound as EB
import test_routes_gpu as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    from lightdiffusion_amd import ops as o
    from lightdiffusion_amd._lib import lib
    lib()
    return o


def _record(case, r, s, **more):
    print(f"ADVERSE {case}: error / bound {r:.3f}, signed bias {s:+.2e}" + "".join(f", {k} {v:.3g}" for k, v in more.items()))
    A.record(case, dict(worst_error_over_bound=round(r, 4), signed_bias_over_tolerance=round(s / EB.BIAS_TOL, 4), **{k: round(float(v), 4) for k, v in more.items()}))


def _pow2(v):
    return 2.0 ** round(math.log2(max(float(v), 1e-30)))


def _rms(t):
    return float(t.double().pow(2).mean().sqrt())


def _rows(table, keys, at):
    """The rows of `table` whose columns `at` equal one of `keys` (each key must name exactly one existing row)."""
    out = []
    for k in keys:
        hit = [row for row in table if tuple(row[i] for i in at) == tuple(k)]
        assert len(hit) == 1, (k, hit)
        out.append(hit[0])
    return out


# ------------------------------------------------------------------ linear

LINEAR_ADVERSE = _rows(R.LINEAR_ROUTES, [
    (200, 192, 72, "gemm4_kernel<64,64,plain>"), (130, 320, 2584, "gemm4_kernel<64,64,plain>+splitk_reduce_kernel"),
    (63, 1280, 328, "gemm4_kernel<64,64,plain>"), (128, 1600, 312, "gemm4_kernel<64,160,plain>"), (2040, 640, 632, "gemm3_kernel<64,64,plain>"),
    (4160, 640, 312, "gemm3_kernel<64,160,plain>"), (300, 640, 64, "gemm4_kernel<64,160,plain>"), (16384, 960, 2560, "gemm5_kernel<256,320,plain>"),
    (24576, 640, 1280, "gemm5_kernel<256,320,geglu>"), (48897, 320, 320, "gemm7_kernel<256,K320,plain>"), (48897, 1280, 320, "gemm7_kernel<256,K320,geglu>"),
    # the text model's fc1 + quick-GELU and fc2 + residual (K = 3072, split over K) at M = 231
    (231, 3072, 768, "gemm4_kernel<64,128,plain>"), (231, 768, 3072, "gemm4_kernel<64,64,plain>+splitk_reduce_kernel"),
], (0, 1, 2, 7))
LINEAR_CASES = [(row, prof, kind) for row in LINEAR_ADVERSE for prof in ("big", "outlier", "heavy") for kind in (("randn", "cancel") if row[4] else ("none",))]


@pytest.mark.parametrize("row,profile,kind", LINEAR_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_linear_adverse(ops, row, profile, kind):
    """y = act(alpha x w^T + bias) + residual with x in `profile`, the bias at the output's magnitude, the residual randn at that magnitude or
    cancelling.  Under `big` the pre-activations of silu / quick_gelu / geglu reach far past 88 (__expf saturates) and the GELU fit's clamp at 6:
    no NaN (EB.check rejects a non-finite output) and the bound."""
    M, N, K, bias, res, act, alpha, route = row
    x, w, b, mag = A.linear_operands(profile, M, N, K, act, 11 + M % 7)
    xd, wd = x.double(), w.double()
    acc, absdot = xd @ wd.t(), xd.abs() @ wd.abs().t()
    pre, _ = EB.epilogue_ref(acc, absdot, K, b, None, alpha, act)
    if profile == "big" and act != "none":
        assert float((alpha * acc + b.double()).abs().max()) > 88.0
    r = None
    if kind == "randn":
        r = (torch.randn(pre.shape, generator=torch.Generator().manual_seed(14)) * _pow2(_rms(pre))).half().to(DEV)
    elif kind == "cancel":
        r = A.cancel(pre)
    y = ops.linear(x, w, b, r, act=act, alpha=alpha)
    assert ops.last_kernel() == route
    # (GEGLU: the value rows are 2^-10, so part of the staged fp16 VALUE tile is subnormal — epilogue_ref's floor max(2^-11 |pre|, 2^-25))
    ref, bound = EB.epilogue_ref(acc, absdot, K, b, r, alpha, act)
    bm = int(route.split("<")[1].split(",")[0]) if not route.startswith("gemm7") else 256
    extra = (EB.GELU_FIT_BIAS if act == "geglu" else 0.0) + (EB.rtn_noise_weighted(pre.abs() + ref.abs(), ref) if kind == "cancel" else 0.0)
    rr, s = EB.check(y, ref, bound, f"{route} {M}x{N}x{K} {act} {profile} residual {kind}", tile=(bm, 160), bias_extra=extra)
    _record(f"linear {route} {M}x{N}x{K} {act} {profile} {kind}", rr, s)


# ------------------------------------------------------------------ the LayerNorm fold

@pytest.mark.parametrize("ratio,scale", A.LN_STATS)
@pytest.mark.parametrize("M,C,N,geglu,route", R.LN_ROUTES, ids=lambda v: str(v))
def test_linear_ln_adverse(ops, M, C, N, geglu, route, ratio, scale):
    """The fold pair on a producer whose bias puts t at mu / sigma = 30 at 2^4 and 8 at 2^7 in every row: t as a plain linear, y element-wise
    against test_routes_gpu._ln_ref (which carries the (acc - mu wsum) cancellation term)."""
    x, wp, bp, gamma, beta, w, b = A.ln_operands(M, C, N, ratio, scale, 21)
    t, y = (ops.linear_ln_geglu if geglu else ops.linear_ln)(x, wp, bp, gamma, beta, w, b)
    assert ops.last_kernel() == route
    td = t[:4096].double()
    got = float((td.mean(-1) / td.std(-1, unbiased=False)).mean())
    assert abs(got / ratio - 1.0) < 0.15, got
    tref, tb = EB.linear_ref(x, wp, bp)
    r0, s0 = EB.check(t, tref, tb, f"{route} producer {M}x{C} mu/sigma {ratio}")
    ref, bound = R._ln_ref(x, wp, bp, gamma, beta, w, b, t, 1e-5, geglu)
    r1, s1 = EB.check(y, ref, bound, f"{route} consumer {M}x{C}x{N} mu/sigma {ratio} at {scale}", bias_extra=EB.GELU_FIT_BIAS if geglu else 0.0)
    _record(f"ln {route} {M}x{C}x{N} mu/sigma {ratio} at {scale}", r1, s1, producer=r0)


def test_linear_ln_constant_rows(ops):
    """Rows of t that are one value repeated (an identity producer hands them over exactly): var = msq - mu^2 is 0 in exact arithmetic and a few
    fp32 ulps of mu^2 either side of it on the device — 1e-2 at |mu| = 500, a thousand times eps — so ln_prepare's clamp at 0 is what keeps rstd
    finite.  With it rstd <= eps^-1/2 and y = beta w^T + bias inside _ln_ref's bound (its cancellation term scales with that rstd); the other rows
    have mu / sigma = 30."""
    M, C, N = R.LN_ROUTES[0][:3]
    g = torch.Generator().manual_seed(31)
    t0 = (torch.randn(M, C, generator=g) + 30.0) * 16.0
    const = torch.arange(M) % 4 == 1
    t0[const] = (470.0 + 0.37 * torch.arange(M, dtype=torch.float32)[const]).unsqueeze(1).expand(-1, C)      # 128 different non-dyadic values
    x = t0.half().to(DEV)
    eye = torch.eye(C).half().to(DEV)
    r = lambda *s, sc=1.0, off=0.0: (torch.randn(*s, generator=g) * sc + off).half().to(DEV)
    gamma, beta, w, b = r(C, sc=0.2, off=1.0), r(C, sc=0.2), r(N, C, sc=1 / math.sqrt(C)), r(N, sc=0.2)
    t, y = ops.linear_ln(x, eye, None, gamma, beta, w, b)
    assert ops.last_kernel() == R.LN_ROUTES[0][4]
    assert torch.equal(t, x)
    ref, bound = R._ln_ref(x, eye, None, gamma, beta, w, b, t, 1e-5, False)
    # the bias statistic over the other rows: a constant row's error is the accumulator's fp32 noise times rstd = eps^-1/2 = 316 (inside the element
    # bound, which scales with that rstd), not a rounding of y
    keep = (~const).to(DEV).unsqueeze(1).expand_as(ref)
    rr, s = EB.check(y, ref, bound, "LN fold with constant rows", keep=keep)
    rc = float(((y.double() - ref).abs() / bound)[const.to(DEV)].max())
    _record("ln constant rows 512x320x320", rr, s, constant_rows=rc)


# ------------------------------------------------------------------ convolutions

CONV_ADVERSE = _rows(R.CONV_ROUTES, [
    (2, 8, 8, 1280, None, "conv8_kernel<W8>"), (2, 64, 64, 320, None, "conv8_kernel<W64>"), (12, 64, 64, 320, None, "conv6_kernel<W64,halo>"),
    (16, 16, 16, 1280, None, "conv6_kernel<W16,halo>+splitk_reduce_kernel"), (2, 11, 9, 320, None, "gemm3_kernel<64,160,conv,deep>+splitk_reduce_kernel"),
    (2, 40, 40, 640, None, "gemm4_kernel<64,64,conv,2wg>"),
], (0, 1, 2, 3, 7, 11))
CONV_CASES = [(row, prof, kind) for row in CONV_ADVERSE for prof in ("big", "outlier") for kind in (("randn", "cancel") if row[10] else ("none",))]


def _conv_mags(x, c, k):
    return _pow2(_rms(x))          # w ~ N(0, 1 / (k^2 C)): the output's standard deviation is the input's rms


@pytest.mark.parametrize("row,profile,kind", CONV_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_conv_adverse(ops, row, profile, kind):
    """NHWC convolution with x (both sources) in `profile`, bias and row vector at the output's magnitude, the residual randn at that magnitude
    or cancelling."""
    n, h, w, c1, c2, cout, stride, out_hw, ksize, rv, res, route = row
    x = A.PROFILES[profile]((n, h, w, c1), 31)
    x2 = A.PROFILES[profile]((n, h, w, c2), 32) if c2 else None
    mag = _conv_mags(x, c1 + c2, ksize)
    wt = R.r16((cout, c1 + c2, ksize, ksize), 33, 1 / math.sqrt(ksize * ksize * (c1 + c2)))
    b = R.r16((cout,), 34, 0.5 * mag)
    rowvec = R.r16((n, cout), 35, 0.5 * mag) if rv else None
    pre, _, (ho, wo) = EB.conv_ref(x, wt, b, None, stride, out_hw, x2, rowvec)
    resid = None
    if kind == "randn":
        resid = R.r16((n, ho, wo, cout), 36, _pow2(_rms(pre)))
    elif kind == "cancel":
        resid = A.cancel(pre).reshape(n, ho, wo, cout)
    y = ops.conv2d(x, ops.repack_conv_weight(wt), b, ksize, stride, x2=x2, out_hw=out_hw, rowvec=rowvec, residual=resid)
    assert ops.last_kernel() == route
    ref, bound, _ = EB.conv_ref(x, wt, b, resid, stride, out_hw, x2, rowvec)
    extra = EB.rtn_noise_weighted(pre.abs() + ref.abs(), ref) if kind == "cancel" else 0.0
    rr, s = EB.check(y.reshape(-1, cout), ref, bound, f"{route} n{n} {h}x{w} c{c1}+{c2}->{cout} {profile} residual {kind}", image_rows=ho * wo, width=wo,
                     bias_extra=extra)
    _record(f"conv {route} n{n} {h}x{w} c{c1}+{c2} {profile} {kind}", rr, s)


@pytest.mark.parametrize("profile", ["big", "outlier"])
@pytest.mark.parametrize("n,h,w,c,sc1,sc2,cout,route", R.SKIP_ROUTES, ids=lambda v: str(v))
def test_conv_skip_adverse(ops, n, h, w, c, sc1, sc2, cout, route, profile):
    """ResBlock's out-conv + 1x1 skip as one contraction, every source in `profile`, both biases at the output's magnitude."""
    x, s1, s2 = (A.PROFILES[profile]((n, h, w, cc), 61 + i) for i, cc in enumerate((c, sc1, sc2)))
    mag = _pow2(_rms(x))
    wt = R.r16((cout, c, 3, 3), 64, 1 / math.sqrt(9 * c + sc1 + sc2))
    wsk = R.r16((cout, sc1 + sc2), 65, 1 / math.sqrt(9 * c + sc1 + sc2))
    b, bsk = R.r16((cout,), 66, 0.5 * mag), R.r16((cout,), 67, 0.5 * mag)
    y = ops.conv2d_skip(x, ops.repack_conv_weight(wt), b, s1, s2, wsk, bsk)
    assert ops.last_kernel() == route
    cols = torch.cat([EB.im2col(x, 3), torch.cat([s1, s2], -1).double().reshape(-1, sc1 + sc2)], 1)
    wm = torch.cat([wt.double().reshape(cout, -1), wsk.double()], 1)
    ref, bound = EB.epilogue_ref(cols @ wm.t(), cols.abs() @ wm.abs().t(), wm.shape[1], b.double() + bsk.double())
    rr, s = EB.check(y.reshape(-1, cout), ref, bound, f"{route} n{n} {h}x{w} {profile}", image_rows=h * w, width=w, tile=(256, 320))
    _record(f"conv_skip {route} {profile}", rr, s)


# ------------------------------------------------------------------ the fused GroupNorm loader

@pytest.mark.parametrize("n,h,w,c1,c2,cout,route", R.GN_CONV_ROUTES, ids=lambda v: str(v))
def test_groupnorm_conv_adverse(ops, n, h, w, c1, c2, cout, route):
    """conv3x3(SiLU(GroupNorm32(cat(x1, x2)))) + bias on groups(...): mu / sigma = +-30, a constant group, a group dominated by one x 64 channel,
    against EB.gn_silu_conv_ref, whose operand error carries groupnorm_ref's cancellation term."""
    C = c1 + c2
    x1, x2, gamma, beta = A.groups(n, h * w, c1, c2, 41)
    x1 = x1.reshape(n, h, w, c1)
    x2 = x2.reshape(n, h, w, c2) if c2 else None
    wt = R.r16((cout, C, 3, 3), 45, 1 / math.sqrt(9 * C))
    b = R.r16((cout,), 46, 0.5)
    y = ops.group_norm_silu_conv2d(x1, gamma, beta, 1e-5, ops.repack_conv_weight(wt), b, x2=x2)
    assert ops.last_kernel().endswith(route)
    ref, bound = EB.gn_silu_conv_ref(x1, gamma, beta, 1e-5, wt, b, x2=x2)
    rr, s = EB.check(y.reshape(-1, cout), ref, bound, f"{route} n{n} {h}x{w} c{c1}+{c2}->{cout} groups", image_rows=h * w, width=w)
    if x2 is None:
        # the fused loader finished from HANDED-OVER partials (here the statistics pass's own, handed in as a producer would): no statistics
        # launch, the same route, the same bound
        y2 = ops.group_norm_silu_conv2d(x1, gamma, beta, 1e-5, ops.repack_conv_weight(wt), b, in_part=ops.group_norm_stats(x1))
        launches = ops.last_launches()
        assert "gn_stats_kernel" not in launches and launches.endswith(route), launches
        r2, _ = EB.check(y2.reshape(-1, cout), ref, bound, f"{route} in_part [{launches}]", image_rows=h * w, width=w)
        print(f"{route}: from handed-over partials [{launches}] error / bound {r2:.3f}, bitwise the own-statistics result: {torch.equal(y2, y)}")
        rr = max(rr, r2)
    _, _, share = EB.groupnorm_ref(x1[:1], None if x2 is None else x2[:1], gamma, beta, 1e-5, True, parts=True)
    _record(f"gn_conv {route} n{n} {h}x{w} c{c1}+{c2}", rr, s, cancellation_share_of_operand_bound=float(share.max()))


# ------------------------------------------------------------------ statistics handed from a producer's epilogue to the next GroupNorm

# producer's route -> the launches of ops.group_norm_silu_conv2d(y, ..., in_part=part) into a 3x3 of the same width.  No gn_stats_kernel anywhere:
# the apply pass runs on the producer's partials.  These widths split over K, so none of them takes the fused loader; that one is held on handed-over
# partials by test_groupnorm_conv_adverse.
HANDOVER_CONSUMER = {
    "gemm3_kernel<64,160,conv,deep>+splitk_reduce_gn_kernel": "gn_apply_kernel;gemm3_kernel<64,160,conv,deep>+splitk_reduce_kernel",
    "gemm3_kernel<64,160,conv>+splitk_reduce_gn_kernel": "gn_apply_kernel;gemm3_kernel<64,160,conv>+splitk_reduce_kernel",
    "gemm3_kernel<128,160,conv>+splitk_reduce_gn_kernel": "gn_apply_kernel;gemm3_kernel<128,160,conv>+splitk_reduce_kernel",
    "conv6_kernel<W32,halo>+splitk_reduce_gn_kernel": "gn_apply_kernel;gemm3_kernel<128,160,conv>+splitk_reduce_kernel",
    "conv6_kernel<W16,halo>+splitk_reduce_gn_kernel": "gn_apply_kernel;conv6_kernel<W16,halo>+splitk_reduce_kernel",
}
assert set(HANDOVER_CONSUMER) == {row[-1] for row in R.GN_PART_ROUTES}


@pytest.mark.parametrize("n,h,w,c,cout,route", R.GN_PART_ROUTES, ids=lambda v: str(v))
def test_handed_over_statistics_adverse(ops, n, h, w, c, cout, route):
    """A producer whose bias puts its output at mu / sigma = +30, -30 and +15 in three groups: the convolution and its partials as
    test_conv_gn_partials_route holds them, then the next GroupNorm finished from those partials — ops.group_norm_from_partials and the fused
    loader of ops.group_norm_silu_conv2d(in_part=...) — against the references of the STORED y.  Where the producer's chunking is gn_stats_kernel's
    own, the two routes to the normalised tensor agree bit for bit; elsewhere both are inside the bound."""
    x = R.r16((n, h, w, c), 51)
    wt = R.r16((cout, c, 3, 3), 52, 1 / math.sqrt(9 * c))
    b = A.group_bias(cout, 53)
    y, part = ops.conv2d_gn_partials(x, ops.repack_conv_weight(wt), b)
    assert ops.last_kernel() == route
    ref, bound, _ = EB.conv_ref(x, wt, b)
    r0, s0 = EB.check(y.reshape(-1, cout), ref, bound, f"{route} n{n} {h}x{w} c{c}->{cout} producer", image_rows=h * w, width=w)
    assert part is not None
    cpg = cout // 32
    yg = y.double().view(n, h * w, 32, cpg)
    ratio = (yg.mean((1, 3)) / yg.std((1, 3), unbiased=False))[:, [A.G_POS, A.G_NEG, A.G_DOM]]
    assert bool((ratio[:, 0] > 25).all() and (ratio[:, 1] < -25).all() and (ratio[:, 2] > 12).all()), ratio.tolist()
    got = part.double().sum(1)
    want = torch.stack([yg.sum((1, 3)), (yg * yg).sum((1, 3))], -1)
    tol = torch.stack([yg.abs().sum((1, 3)), (yg * yg).sum((1, 3))], -1) * (EB.c_acc(h * w * cpg) + 2.0 ** -22) + EB.TINY
    assert bool(((got - want).abs() <= tol).all()), float(((got - want).abs() / tol).max())
    g = torch.Generator().manual_seed(54)
    gamma = (1.0 + 0.5 * torch.randn(cout, generator=g)).half().to(DEV)
    beta = (0.5 * torch.randn(cout, generator=g)).half().to(DEV)
    own = ops.group_norm_stats(y)
    same_chunks = own.shape == part.shape
    worst = 0.0
    for silu in (False, True):
        nref, nbound, share = EB.groupnorm_ref(y, None, gamma, beta, 1e-5, silu, parts=True)
        handed = ops.group_norm_from_partials(y, part, gamma, beta, 1e-5, silu)
        mine = ops.group_norm_from_partials(y, own, gamma, beta, 1e-5, silu)
        r1, s1 = EB.check(handed.reshape(nref.shape), nref, nbound, f"{route}: group_norm_from_partials(producer's) silu={silu}")
        r2, _ = EB.check(mine.reshape(nref.shape), nref, nbound, f"{route}: group_norm_from_partials(own) silu={silu}")
        worst = max(worst, r1, r2)
        if same_chunks:
            assert torch.equal(handed, mine), f"{route}: the producer's chunking is gn_stats_kernel's, yet {int((handed != mine).sum())} outputs differ"
        print(f"{route}: producer chunks {part.shape[1]}, gn_stats chunks {own.shape[1]}, partials bitwise equal {same_chunks and torch.equal(part, own)}, "
              f"outputs bitwise equal {torch.equal(handed, mine)} ({int((handed != mine).sum())} of {handed.numel()} differ)")
    w2 = R.r16((cout, cout, 3, 3), 55, 1 / math.sqrt(9 * cout))
    b2 = R.r16((cout,), 56, 0.5)
    z = ops.group_norm_silu_conv2d(y, gamma, beta, 1e-5, ops.repack_conv_weight(w2), b2, in_part=part)
    consumer = ops.last_launches()
    assert consumer == HANDOVER_CONSUMER[route], f"{route}: the consumer of the handed-over partials ran {consumer}"
    zref, zbound = EB.gn_silu_conv_ref(y, gamma, beta, 1e-5, w2, b2)
    r3, s3 = EB.check(z.reshape(-1, cout), zref, zbound, f"{route}: group_norm_silu_conv2d(in_part) [{ops.last_kernel()}]", image_rows=h * w, width=w)
    _record(f"gn_handover {route}", max(worst, r3), s3, producer=r0, norm_from_partials=worst, cancellation_share=float(share.max()))


# ------------------------------------------------------------------ attention: V at magnitude (peaked scores: test_attention_route_peaked)

ATTN_ADVERSE = _rows(R.ATTN_ROUTES, [(False, 100, 128, 40, False), (False, 77, 77, 64, True), (True, 200, 161, 512, False)], (0, 3, 4, 5, 6))


@pytest.mark.parametrize("profile", ["big", "outlier"])
@pytest.mark.parametrize("rowv,b,heads,lq,lk,d,causal,route", ATTN_ADVERSE, ids=lambda v: str(v))
def test_attention_adverse_v(ops, rowv, b, heads, lq, lk, d, causal, route, profile):
    q, k = R.r16((b, lq, heads * d), 1), R.r16((b, lk, heads * d), 2)
    v = A.PROFILES[profile]((b, lk, heads * d), 3)
    o = R._attn_call(ops, rowv, q, k, v, heads, causal)
    assert ops.last_kernel() == route
    ref, bound = EB.attention_ref(q, k, v, heads, causal)
    rr, s = EB.check(o, ref, bound, f"{route} V {profile}")
    _record(f"attention {route} Lq{lq} Lk{lk} d{d} V {profile}", rr, s)


# ------------------------------------------------------------------ small kernels

@pytest.mark.parametrize("c", [320, 768])
def test_layernorm_adverse(ops, c):
    """layernorm_kernel on rows with mu / sigma = 30 at 2^4 (its two passes have no cancellation term; what remains is e_mu)."""
    g = torch.Generator().manual_seed(c)
    x = A.mean((130, c), c)
    ga, be = (1.0 + 0.5 * torch.randn(c, generator=g)).half().to(DEV), (0.5 * torch.randn(c, generator=g)).half().to(DEV)
    y = ops.layer_norm(x, ga, be, 1e-5)
    ref, bound = EB.layernorm_ref(x, ga, be, 1e-5)
    rr, s = EB.check(y, ref, bound, f"layernorm C={c} mean", bias_extra=EB.rtn_noise(EB.independent_roundings(ref)))
    _record(f"layernorm C={c} mean", rr, s)


@pytest.mark.parametrize("cols", [40, 2056])
def test_softmax_adverse(ops, cols):
    """softmax_rows on rows whose scores span -6e4 .. +6e4 (the maximum near +6e4 with a few columns within a few units of it, the rest
    underflows to exact zeros)."""
    g = torch.Generator().manual_seed(cols)
    rows = 300
    s = (torch.rand(rows, cols, generator=g) * 2.0 - 1.0) * 6.0e4
    top = torch.randint(0, cols, (rows, 6), generator=g)
    s.scatter_(1, top, 6.0e4 - torch.rand(rows, 6, generator=g) * 64.0)
    s = s.half().to(DEV)
    ref, bound = EB.softmax_ref(s)
    y = ops.softmax_rows_(s.clone())
    keep = ref > 2.0 ** -14
    rr, sb = EB.check(y, ref, bound, f"softmax +-6e4 cols={cols}", keep=keep, bias_extra=EB.rtn_noise(EB.independent_roundings(ref, keep)))
    assert bool((y[ref < 2.0 ** -30] == 0).all())
    _record(f"softmax +-6e4 cols={cols}", rr, sb)


def test_small_conv_in_adverse(ops):
    """small_conv_in (sigma variant) on latents times 2^6."""
    g = torch.Generator().manual_seed(7)
    n, cin, h, w, cout = 2, 4, 16, 12, 320
    x = (torch.randn(n, cin, h, w, generator=g) * 64.0).to(DEV)
    wt, b = (torch.randn(cout, 9 * cin, generator=g) / 6.0).half().to(DEV), (torch.randn(cout, generator=g) * 32.0).half().to(DEV)
    sig = torch.tensor([14.6, 0.03], dtype=torch.float32, device=DEV)
    y = ops.small_conv_in(x, wt, b, sig)
    assert ops.last_kernel().startswith("small_conv_in_kernel")
    ref, bound = EB.small_conv_in_ref(x, wt, b, scale_sigma=sig)
    rr, s = EB.check(y.reshape(ref.shape), ref, bound, "small_conv_in sigma latents x 2^6", image_rows=h * w, width=w)
    _record("small_conv_in sigma x64", rr, s)


# ------------------------------------------------------------------ the store past 65504

LO, HI = 65504.0 * (1.0 - 2.0 ** -9), 65520.0 * (1.0 + 2.0 ** -9)


def _resid(shape, seed):
    """A residual at 2^14, clamped inside fp16's range (no operand of the policy cases is an infinity)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(tuple(shape), generator=g) * 2.0 ** 14).clamp(-6.0e4, 6.0e4).half().to(DEV)


def _ramp(n, lo, hi):
    """2^lo .. 2^hi, increasing along the n output columns."""
    return torch.exp2(lo + (hi - lo) * torch.arange(n, dtype=torch.float64) / max(1, n - 1)).to(DEV)


def _policy(y, stages, ref, bound, what):
    """stages: the fp64 values of the fp16 roundings an element passes, in order (the last is the store).  Safe elements (every stage below LO)
    are finite and inside the bound; an element with a stage above HI is +-inf with the sign of its first such stage; the band between is left out
    and holds under 1 % of the case (asserted on the fp64 reference alone); no NaN anywhere (no operand here is an infinity, so no add meets an
    opposite one); every safe element that shares a row with an inf is inside its bound like any other."""
    y = y.double().reshape(ref.shape)
    assert all(bool(torch.isfinite(s).all()) for s in stages), f"{what}: an operand is not finite"
    mags = torch.stack([s.abs() for s in stages])
    safe = (mags < LO).all(0)
    over = (mags > HI).any(0)
    band = ~safe & ~over
    frac = float(band.double().mean())
    assert frac < 0.01, f"{what}: {frac:.3%} of the elements lie between the thresholds"
    assert int(over.sum()) > 0 and float(safe.double().mean()) > 0.2, f"{what}: the ramp does not straddle the range"
    assert not bool(torch.isnan(y).any()), f"{what}: {int(torch.isnan(y).sum())} NaN"
    first = torch.zeros_like(ref)
    for s in reversed(stages):
        first = torch.where(s.abs() > HI, s.sign(), first)
    bad = over & (y != first * float("inf"))
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {int(over.sum())} overflowed elements are not the infinity of their stage, e.g. "
                                 f"{EB.locate(int(bad.flatten().nonzero()[0]), tuple(ref.shape))}: {float(y.flatten()[bad.flatten().nonzero()[0]])}")
    assert bool(torch.isfinite(y[safe]).all()), f"{what}: {int((~torch.isfinite(y[safe])).sum())} in-range elements are not finite"
    ratio = ((y - ref).abs() / bound)[safe]
    assert float(ratio.max()) <= 1.0, f"{what}: an in-range element is outside its bound, error / bound {float(ratio.max()):.3g}"
    rows_with_inf = over.reshape(-1, ref.shape[-1]).any(-1)
    beside = safe.reshape(-1, ref.shape[-1]) & rows_with_inf.unsqueeze(-1)
    assert int(beside.sum()) > 0
    print(f"OVERFLOW {what}: {int(over.sum())} inf, {int(safe.sum())} in range (worst error / bound {float(ratio.max()):.3f}), {frac:.3%} left out, "
          f"{int(beside.sum())} in-range elements share a row with an inf")


POLICY = ["plain", "bias_residual", "silu", "quick_gelu", "geglu", "splitk", "ln_consumer", "conv6_halo", "gn_apply"]
# family -> (M, N, K, act, alpha, expected route): rows of LINEAR_ROUTES
POLICY_LINEAR = {"plain": (200, 192, 72, "none", 1.0, "gemm4_kernel<64,64,plain>"), "bias_residual": (200, 192, 72, "none", 1.0, "gemm4_kernel<64,64,plain>"),
                 "silu": (63, 1280, 328, "silu", 1.0, "gemm4_kernel<64,64,plain>"), "quick_gelu": (128, 1600, 312, "quick_gelu", 1.0, "gemm4_kernel<64,160,plain>"),
                 "geglu": (300, 640, 64, "geglu", 1.0, "gemm4_kernel<64,160,plain>"), "splitk": (130, 320, 2584, "none", 0.75, "gemm4_kernel<64,64,plain>+splitk_reduce_kernel")}


@pytest.mark.parametrize("family", POLICY)
def test_overflow_policy(ops, family):
    """What a store does past 65504, per epilogue family, on operands whose magnitude increases along the output columns (the weight rows carry
    a ramp), in the stage order EB.epilogue_ref models: the staged tile, after the row vector, after the residual.  Every family asserts its route.
    SiLU / quick-GELU run in both signs: a staged tile that overflowed to -inf is absorbed by the activation — its true value there is -0, which
    the tile epilogues return (common.h silu_tile_f; -inf / (1 + inf) was NaN) as the fp32 direct-store path does — so such an element counts as
    in range: finite and inside its bound, which is the residual's.  A positive overflow stays +inf."""
    g = torch.Generator().manual_seed(len(family))
    rn = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc)
    if family in POLICY_LINEAR:
        M, N, K, act, alpha, route = POLICY_LINEAR[family]
        x = rn(M, K, sc=32.0)                  # 2^5 on x, 2^5 .. 2^13 on the weight rows: every operand stays far inside fp16's range
        w = rn(N, K, sc=1 / math.sqrt(K)).double()
        n_out = N // 2 if act == "geglu" else N
        w[:n_out] *= _ramp(n_out, 5.0, 13.0).cpu().unsqueeze(1)
        b = rn(N, sc=4.0) if family != "plain" else None
        if act == "geglu":                     # the gate is 2 everywhere: gelu(2) = 1.954, the value half carries the ramp
            w[n_out:] = 0.0
            b[n_out:] = 2.0
        x, w = x.half().to(DEV), w.half().to(DEV)
        b = None if b is None else b.half().to(DEV)
        r = _resid((M, n_out), 15) if family in ("bias_residual", "silu", "quick_gelu") else None
        y = ops.linear(x, w, b, r, act=act, alpha=alpha)
        assert ops.last_kernel() == route
        xd, wd = x.double(), w.double()
        acc, absdot = xd @ wd.t(), xd.abs() @ wd.abs().t()
        ref, bound = EB.epilogue_ref(acc, absdot, K, b, r, alpha, act)
        pre = alpha * acc + (0.0 if b is None else b.double())
        if act == "geglu":
            a, ga = pre[:, :n_out], EB._act(pre[:, n_out:], "gelu")
            stages = [a, a * ga]
        else:
            ya = EB._act(pre, act)
            tile = pre
            if act != "none":                  # a negative overflow of the tile is absorbed: act(-inf) = -0
                absorbed = pre < -HI
                assert int(absorbed.sum()) > 100, f"{family}: no pre-activation below -65520"
                assert bool((y[absorbed].float() == r[absorbed].float()).all()), f"{family}: act(-inf) + r is not r"
                tile = pre.clamp_min(0.0)
            stages = [tile, ya] + ([ya + r.double()] if r is not None else [])
        _policy(y, stages, ref, bound, f"{family} [{route}]")
    elif family == "ln_consumer":
        M, C, N = R.LN_ROUTES[0][:3]
        x, wp, bp, gamma, beta, w, b = A.ln_operands(M, C, N, 8.0, 16.0, 5)
        w = (w.double() * _ramp(N, 10.0, 17.0).unsqueeze(1)).half()      # (2^17: the folded weights half(gamma w) stay finite)
        assert bool(torch.isfinite(w.float() * gamma.float()).all()) and float((w.float() * gamma.float()).abs().max()) < 6.0e4
        t, y = ops.linear_ln(x, wp, bp, gamma, beta, w, b)
        assert ops.last_kernel() == R.LN_ROUTES[0][4]
        ref, bound = R._ln_ref(x, wp, bp, gamma, beta, w, b, t, 1e-5, False)
        _policy(y, [ref], ref, bound, f"ln_consumer [{R.LN_ROUTES[0][4]}]")
    elif family == "conv6_halo":
        n, h, w_, c, cout = 12, 64, 64, 320, 320
        x = R.r16((n, h, w_, c), 71, 32.0)
        wt = (R.r16((cout, c, 3, 3), 72, 1 / math.sqrt(9 * c)).double() * _ramp(cout, 5.0, 13.0).reshape(-1, 1, 1, 1)).half()
        b, rowvec = R.r16((cout,), 73, 4.0), R.r16((n, cout), 74, 4.0)
        resid = _resid((n, h, w_, cout), 75)
        y = ops.conv2d(x, ops.repack_conv_weight(wt), b, 3, 1, rowvec=rowvec, residual=resid)
        assert ops.last_kernel() == "conv6_kernel<W64,halo>"
        ref, bound, _ = EB.conv_ref(x, wt, b, resid, 1, None, None, rowvec)
        rv = rowvec.double().repeat_interleave(h * w_, dim=0)
        rs = resid.double().reshape(-1, cout)
        _policy(y, [ref - rs - rv, ref - rs, ref], ref, bound, "conv6_halo [conv6_kernel<W64,halo>]")
    else:
        n, hw, c = 2, 77, 320
        x1, _, ga, be = R.r16((n, hw, c), 81), None, (R.r16((c,), 82, 0.2, 1.0).double() * _ramp(c, 9.0, 15.0)).half(), R.r16((c,), 83, 4.0)
        for silu in (False, True):
            y = ops.group_norm(x1, ga, be, 1e-5, silu)
            assert ops.last_launches() == "gn_stats_kernel+gn_apply_kernel", ops.last_launches()
            ref, bound = EB.groupnorm_ref(x1, None, ga, be, 1e-5, silu)
            _policy(y, [ref], ref, bound, f"gn_apply silu={silu} [gn_stats_kernel+gn_apply_kernel]")


def test_axpby_has_no_fp16_stage(ops):
    """axpby_ works on fp32 latents: a value past 65504 is an ordinary number there — finite, and exact to fp32 rounding (no fp16 intermediate)."""
    g = torch.Generator().manual_seed(3)
    n = 4096
    x, yv, z = (torch.randn(n, generator=g).double() * _ramp(n, 10.0, 20.0).cpu() for _ in range(3))
    x32, y32, z32 = (t.float().to(DEV) for t in (x, yv, z))
    ref = 0.5 * x32.double() - 2.0 * y32.double() + 0.25 * z32.double()
    out = ops.axpby_(x32.clone(), 0.5, y32, -2.0, z32, 0.25).double()
    assert bool(torch.isfinite(out).all()) and float(ref.abs().max()) > 4 * 65504.0
    mag = 0.5 * x32.double().abs() + 2.0 * y32.double().abs() + 0.25 * z32.double().abs()
    assert bool(((out - ref).abs() <= 2.0 ** -22 * mag).all())
