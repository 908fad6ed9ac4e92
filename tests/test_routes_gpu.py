"""Route-pinned, element-wise parity of every reachable contraction instantiation.

Each row of the tables below names an operator call, a shape on the edge of a dispatch rule, and the kernel instantiation(s) that call must
dispatch (`ops.last_kernel()`, the names of the profile tables).  A test asserts the route string exactly, then holds every output element to
the bound of tests/errbound.py against an fp64 reference of the same fp16 inputs (on the device; plus a CPU fp64 evaluation of rows that cover
every tile-boundary class), then the signed-bias statistic.  A retuned threshold that moves a shape to another kernel fails here by name, and
the route it moved to has to get its own row.

Bounds (tests/errbound.py): |y - y_hat| <= 2^-11 |y_hat| + c_acc(K) |A| |W| + L_act (2^-23 |pre| + ...) + eps_act + 2^-24, plus per extra fp16
rounding of an operand (GroupNorm-normalised loader, LayerNorm-folded weights, attention's scaled Q and P) 2^-11 of that operand propagated;
|mean signed error| / mean |y_hat| <= 2^-11 / 8 (+ the GELU fit's documented bias for GEGLU).

ATTN_PEAKED / test_attention_route_peaked: randn inputs at scale 1 never move the attention's lazy softmax reference after the first 32-key
subtile, so the rescale arm of flash_attn2_kernel / flash_attn512_kernel (O and l scaled, scores shifted, the MFMA's C operand rewritten) ran in
no row of ATTN_ROUTES.  The peaked table runs every attention instantiation of ATTN_ROUTES on the inputs of tests/attn_patterns.py, whose moves an
fp64 run of the recursion records and whose margins keep them independent of rounding: spike (one planted key per row in a later subtile, 6 / 10 /
20 / 40 units above the reference, every position of the subtile, a flat row beside every two peaked ones), stairs (a move in every subtile),
descend (all weight in the first subtile, the rest underflows in P), offset (every score of a row +-35 units away from zero), onehot (one key
40 units above all others: the output row is that key's v row bit for bit).  Same route assertion, same element bound.
"""
import functools
import math

import pytest
import torch

import errbound as EB

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    from lightdiffusion_amd import ops as o
    from lightdiffusion_amd._lib import lib
    lib()
    return o


def r16(shape, seed, scale=1.0, offset=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale + offset).half().to(DEV)


# ------------------------------------------------------------------ attention: every head-dim class x V layout x plain / masked x 4 / 8 waves

def _fa2(dk, rowv, masked, nw):
    return f"flash_attn2_kernel<{dk}{',rowV' if rowv else ''},{'masked' if masked else 'plain'},{nw}>"


# (V layout, b, heads, Lq, Lk, d, causal, expected route).  Lq = 100 / 200 end inside a 128-query workgroup; Lk % 64 in {0, 1, 63};
# d = 24 / 56 / 72 / 88 / 120 / 152 leave a tail inside their k-step class; even DK (d in 17-32, 49-64, 81-96, 113-128, 145-160) have no
# spare V column for the ones trick: their softmax denominator is summed in a register, from the rounded weights the MFMA multiplies.
ATTN_ROUTES = []
for _d, _dk in [(8, 1), (16, 1), (24, 2), (32, 2), (40, 3), (48, 3), (56, 4), (64, 4), (72, 5), (80, 5), (88, 6), (96, 6),
                (120, 8), (128, 8), (152, 10), (160, 10)]:
    for _rowv in (False, True):
        ATTN_ROUTES.append((_rowv, 2, 2, 100, 128, _d, False, _fa2(_dk, _rowv, False, 4)))
        ATTN_ROUTES.append((_rowv, 1, 2, 200, 65 if _d % 16 else 127, _d, False, _fa2(_dk, _rowv, True, 4)))
for _d, _dk in [(40, 3), (64, 4)]:
    for _rowv in (False, True):
        # 8-wave workgroups: DK <= 4, Lq >= 2048 and >= 512 256-query blocks
        ATTN_ROUTES.append((_rowv, 8, 8, 2048, 64, _d, False, _fa2(_dk, _rowv, False, 8)))
        ATTN_ROUTES.append((_rowv, 8, 8, 2048, 63, _d, False, _fa2(_dk, _rowv, True, 8)))
        # one block short of the 8-wave rule: 4 waves
        ATTN_ROUTES.append((_rowv, 8, 8, 1920, 64, _d, False, _fa2(_dk, _rowv, False, 4)))
for _d, _dk in [(40, 3), (64, 4)]:
    for _rowv in (False, True):
        # 8-wave workgroups that END inside their 256 queries: Lq = 2112 is 8 blocks and 64 queries, six of the last block's eight waves hold no
        # query; 33 full key tiles (self-attention), and the 77 keys of a prompt
        ATTN_ROUTES.append((_rowv, 8, 8, 2112, 2112, _d, False, _fa2(_dk, _rowv, False, 8)))
        ATTN_ROUTES.append((_rowv, 8, 8, 2112, 77, _d, False, _fa2(_dk, _rowv, True, 8)))
for _d, _dk in [(64, 4), (160, 10)]:
    ATTN_ROUTES.append((False, 1, 2, 77, 77, _d, True, _fa2(_dk, False, True, 4)))        # causal (CLIP: d = 64, L = 77)
    ATTN_ROUTES.append((True, 1, 2, 128, 128, _d, True, _fa2(_dk, True, True, 4)))
for _D in (256, 512):
    ATTN_ROUTES.append((True, 2, 1, 256, 256, _D, False, f"flash_attn512_kernel<{_D},plain>"))
    ATTN_ROUTES.append((True, 1, 1, 200, 161, _D, False, f"flash_attn512_kernel<{_D},masked>"))
    ATTN_ROUTES.append((True, 1, 1, 192, 192, _D, True, f"flash_attn512_kernel<{_D},masked>"))


def _attn_call(ops, rowv, q, k, v, heads, causal):
    return (ops.attention_rowv if rowv else ops.attention)(q, k, v, heads, causal=causal)


@pytest.mark.parametrize("rowv,b,heads,lq,lk,d,causal,route", ATTN_ROUTES, ids=lambda v: str(v))
def test_attention_route(ops, rowv, b, heads, lq, lk, d, causal, route):
    """Route, element-wise bound and bias of the attention against fp64 softmax(q k^T / sqrt(d)) v (errbound.attention_ref: output rounding
    and P's fp16 rounding 2^-11 each, the scaled-Q rounding through the scores' sensitivity, fp32 accumulation)."""
    q, k, v = r16((b, lq, heads * d), 1), r16((b, lk, heads * d), 2), r16((b, lk, heads * d), 3)
    o = _attn_call(ops, rowv, q, k, v, heads, causal)
    assert ops.last_kernel() == route
    ref, bound = EB.attention_ref(q, k, v, heads, causal)
    EB.check(o, ref, bound, f"{route} b{b} h{heads} Lq{lq} Lk{lk} d{d}")


@pytest.mark.parametrize("rowv,b,heads,lq,lk,d,causal,route", ATTN_ROUTES, ids=lambda v: str(v))
def test_attention_constant_v_is_exact(ops, rowv, b, heads, lq, lk, d, causal, route):
    """V == 1: every output is a weighted mean of ones.  Numerator and denominator sum the same fp16-rounded weights (the ones column, or
    l_run), so every instantiation returns exactly 1.0 from 64 keys on.  Below 64 keys (a causal row sees fewer) a handful of weights can move
    it one fp16 ulp.  Truncated P against an unrounded denominator returned 0.99951 in every row; P rounded to nearest against an unrounded
    denominator (the weighted mean of +-2^-11 errors: inside the half ulp 2^-12 below 1.0 while many keys share the weight) still did in the
    ONE row of 135168 that two keys dominate — d = 64, 2112 queries, 77 keys, effective key count 2.3 — until l_run summed the rounded weights."""
    q, k = r16((b, lq, heads * d), 4), r16((b, lk, heads * d), 5)
    v = torch.ones(b, lk, heads * d, dtype=torch.float16, device=DEV)
    o = _attn_call(ops, rowv, q, k, v, heads, causal).float()
    assert ops.last_kernel() == route
    if causal:
        keys = torch.arange(1, lq + 1, device=DEV).view(1, lq, 1).expand_as(o)
        exact = keys >= 64
        assert bool((o[exact] == 1.0).all()), f"{route}: V == 1 gave {o[exact].min().item():.6f} .. {o[exact].max().item():.6f}"
        assert float((o[~exact] - 1.0).abs().max()) <= 2.0 ** -10
    elif lk >= 64:
        assert bool((o == 1.0).all()), f"{route}: V == 1 gave {o.min().item():.6f} .. {o.max().item():.6f}"
    else:
        assert float((o - 1.0).abs().max()) <= 2.0 ** -10


def test_attention_unsupported_head_dims_rejected(ops):
    """d = 104..112 / 136..144 (k-step classes 7 / 9) have no instantiation: LD_ERR_SHAPE, nothing dispatched (no eager fall-back)."""
    from lightdiffusion_amd._lib import LDError
    for d in (112, 136, 168):
        q = r16((1, 64, d), 6)
        with pytest.raises(LDError):
            ops.attention(q, q, q, 1)
        assert ops.last_kernel() == ""


# ------------------------------------------------------------------ attention under peaked scores: the lazy softmax rescale per route

# (seam, b, heads, Lq, Lk, d, causal, expected route, patterns).  seam: 'vt' ops.attention (transposed V), 'rowv' ops.attention_rowv,
# 'qkv' ops.attention_qkv (row pitch 3C, one batch stride).  The shapes are the smallest that cross a 64-key tile boundary with a move:
# Lk = 192 is three full tiles, Lk = 161 leaves 33 keys in the last tile, one valid key alone in its second subtile.
ALL_PATTERNS = ("spike", "stairs", "descend", "offset", "onehot")
ATTN_PEAKED = []
for _d, _dk in [(8, 1), (16, 1), (24, 2), (32, 2), (40, 3), (48, 3), (56, 4), (64, 4), (72, 5), (80, 5), (88, 6), (96, 6),
                (120, 8), (128, 8), (152, 10), (160, 10)]:
    for _rowv in (False, True):
        _seam = "rowv" if _rowv else "vt"
        ATTN_PEAKED.append((_seam, 2, 2, 100, 192, _d, False, _fa2(_dk, _rowv, False, 4), ALL_PATTERNS))
        ATTN_PEAKED.append((_seam, 1, 2, 200, 161, _d, False, _fa2(_dk, _rowv, True, 4), ALL_PATTERNS))
for _d, _dk in [(64, 4), (160, 10)]:
    ATTN_PEAKED.append(("vt", 1, 2, 77, 77, _d, True, _fa2(_dk, False, True, 4), ALL_PATTERNS))
    ATTN_PEAKED.append(("rowv", 1, 2, 128, 128, _d, True, _fa2(_dk, True, True, 4), ALL_PATTERNS))
for _D in (256, 512):
    ATTN_PEAKED.append(("rowv", 2, 1, 256, 256, _D, False, f"flash_attn512_kernel<{_D},plain>", ALL_PATTERNS))
    ATTN_PEAKED.append(("rowv", 1, 1, 200, 161, _D, False, f"flash_attn512_kernel<{_D},masked>", ALL_PATTERNS))
    ATTN_PEAKED.append(("rowv", 1, 1, 192, 192, _D, True, f"flash_attn512_kernel<{_D},masked>", ALL_PATTERNS))
for _d, _dk in [(40, 3), (64, 4)]:
    for _rowv in (False, True):
        # 8-wave workgroups (the fp64 reference of one case is a few GB): two patterns
        ATTN_PEAKED.append(("rowv" if _rowv else "vt", 8, 8, 2048, 192, _d, False, _fa2(_dk, _rowv, False, 8), ("spike", "onehot")))
        ATTN_PEAKED.append(("rowv" if _rowv else "vt", 8, 8, 2048, 191, _d, False, _fa2(_dk, _rowv, True, 8), ("spike", "onehot")))
for _d, _dk in [(40, 3), (80, 5), (160, 10)]:
    ATTN_PEAKED.append(("qkv", 2, 8, 192, 192, _d, False, _fa2(_dk, True, False, 4), ("spike", "stairs")))       # the executors' own layout
ATTN_PEAKED.append(("qkv", 2, 1, 256, 256, 512, False, "flash_attn512_kernel<512,plain>", ("spike", "stairs")))
for _d, _dk in [(40, 3), (64, 4)]:
    for _lk, _masked in ((2112, False), (77, True)):
        for _rowv in (False, True):
            # the 8-wave workgroup that ends inside its 256 queries (ATTN_ROUTES); the two V layouts of a shape side by side: they share inputs
            ATTN_PEAKED.append(("rowv" if _rowv else "vt", 8, 8, 2112, _lk, _d, False, _fa2(_dk, _rowv, _masked, 8), ("spike", "onehot")))
ATTN_PEAKED_CASES = [row[:8] + (pat,) for row in ATTN_PEAKED for pat in row[8]]


@functools.lru_cache(maxsize=2)
def _peaked_inputs(pattern, b, heads, lq, lk, d, causal):
    """attn_patterns.make on the CPU (never changed by a test); the last two kept: the V layouts of one shape run on the same inputs, and the
    fp64 recursion of a 2112 x 2112 case takes longer than its kernel and reference together."""
    import attn_patterns as AP
    return AP.make(pattern, b, heads, lq, lk, d, causal, seed=d)


@pytest.mark.parametrize("seam,b,heads,lq,lk,d,causal,route,pattern", ATTN_PEAKED_CASES, ids=lambda v: str(v))
def test_attention_route_peaked(ops, seam, b, heads, lq, lk, d, causal, route, pattern):
    """The same route, element bound and bias statistic as test_attention_route on inputs whose softmax reference moves after the first subtile
    (tests/attn_patterns.py), and the onehot rows bit for bit."""
    import attn_patterns as AP
    q, k, v, facts = (t.to(DEV) if isinstance(t, torch.Tensor) else t for t in _peaked_inputs(pattern, b, heads, lq, lk, d, causal))
    if seam == "qkv":
        o = ops.attention_qkv(torch.cat([q, k, v], -1).contiguous(), heads, causal=causal)
    else:
        o = _attn_call(ops, seam == "rowv", q, k, v, heads, causal)
    assert ops.last_kernel() == route
    ref, bound = EB.attention_ref(q, k, v, heads, causal, p_subnormal=True)
    what = f"{route} {seam} {pattern} b{b} h{heads} Lq{lq} Lk{lk} d{d}"
    same = AP.onehot_rows_equal_v(o, v, heads, facts)
    try:
        r, s = EB.check(o, ref, bound, what)
    except AssertionError as e:
        raise AssertionError(f"{e}\n{_peaked_context(str(e), facts, heads, d)}") from None
    print(f"PEAKED {what}: error / bound {r:.3f}, signed bias {s:.2e}, rows with a late move "
          f"{float(facts['moves'].any(-1).double().mean()):.2f}")
    assert same is True, f"{what}: onehot rows differ from their key's v row (b, head, row, key): {facts['onehot'][~same.cpu()].tolist()}"


def _peaked_context(msg, facts, heads, d):
    """The recursion's facts of the query that errbound.check named as the worst element ('element (b, row, column)')."""
    import re
    m = re.search(r"element \((\d+), (\d+), (\d+)\)", msg)
    if m is None:
        return ""
    bi, row, col = (int(x) for x in m.groups())
    mv, gp = facts["moves"][bi, col // d, row], facts["gaps"][bi, col // d, row]
    return (f"query (b {bi}, head {col // d}, row {row}): reference moves in subtiles {mv.nonzero().flatten().tolist()}, "
            f"subtile maximum minus reference {[round(float(x), 2) for x in gp]}")


# ------------------------------------------------------------------ linear (ld_op_linear / ld_op_linear_ln*)

# (M, N, K, bias, residual, act, alpha, expected route).  K % 64 in {8, 24, 56} where the route allows; M ragged against the tile height.
LINEAR_ROUTES = [
    # skinny: <= 256 64x160 tiles and <= 8 column tiles -> 64 x 64 producer / consumer kernel
    (200, 192, 72, True, True, "none", 1.0, "gemm4_kernel<64,64,plain>"),
    (130, 320, 2584, True, False, "none", 0.75, "gemm4_kernel<64,64,plain>+splitk_reduce_kernel"),      # K / 640 caps the split at 4
    (63, 1280, 328, True, False, "silu", 1.0, "gemm4_kernel<64,64,plain>"),
    (2040, 640, 648, True, True, "none", 1.0, "gemm4_kernel<64,64,plain,2wg>"),                       # 320 blocks, K >= 640
    (2040, 640, 632, True, True, "none", 1.0, "gemm3_kernel<64,64,plain>"),                          # K < 640: no 2wg
    (128, 1600, 312, True, False, "quick_gelu", 1.0, "gemm4_kernel<64,160,plain>"),                  # 10 column tiles: keeps 160
    (128, 1600, 1304, True, True, "none", 1.0, "gemm4_kernel<64,160,plain>+splitk_reduce_kernel"),
    (200, 1152, 72, False, False, "none", 1.0, "gemm4_kernel<64,128,plain>"),                        # N on 128, not 160
    (2048, 2560, 640, True, False, "none", 1.0, "gemm4_kernel<128,160,plain>"),                      # exactly 256 blocks
    (2049, 2560, 640, True, False, "none", 1.0, "gemm3_kernel<128,160,plain>"),                      # one tile row more
    (2048, 2048, 632, False, True, "none", 1.0, "gemm4_kernel<128,128,plain>"),
    (4160, 640, 312, True, True, "silu", 1.0, "gemm3_kernel<64,160,plain>"),
    (2048, 1152, 200, True, False, "none", 1.0, "gemm3_kernel<64,128,plain>"),
    (4096, 1152, 200, True, False, "none", 1.0, "gemm3_kernel<128,128,plain>"),
    (1024, 2560, 4096, True, True, "none", 1.0, "gemm3_kernel<128,160,plain>+splitk_reduce_kernel"),
    (3968, 2560, 1280, True, False, "none", 1.0, "gemm3_kernel<128,160,plain>"),                     # split 2 does not fit the scratch
    # 256 x 320 tiles once 192 of them fill the chip (K >= 2560)
    (16384, 960, 2560, True, True, "none", 1.0, "gemm5_kernel<256,320,plain>"),
    (16127, 960, 2560, True, True, "none", 1.0, "gemm3_kernel<128,160,plain>"),                      # 189 tiles
    (24576, 640, 1280, True, False, "geglu", 1.0, "gemm5_kernel<256,320,geglu>"),
    # K = 320 row panels once 192 of them fill the chip
    (48897, 320, 320, True, True, "none", 1.0, "gemm7_kernel<256,K320,plain>"),
    (48896, 320, 320, True, True, "none", 1.0, "gemm3_kernel<128,160,plain>"),                       # 191 panels
    (48897, 1280, 320, True, False, "geglu", 1.0, "gemm7_kernel<256,K320,geglu>"),
    (4096, 1280, 320, True, False, "geglu", 1.0, "gemm4_kernel<128,160,plain>"),
    (300, 640, 64, True, False, "geglu", 1.0, "gemm4_kernel<64,160,plain>"),
    # the CLIP-L text model's four contractions (qkv, out-proj + residual, fc1 + quick-GELU, fc2 + residual) at M = 77 B: one prompt, and B = 3
    # (M = 231 ends 25 rows into its fourth 64-row tile).  Appended: tests/test_adverse_routes_gpu.py names rows of this table
    (77, 2304, 768, True, False, "none", 1.0, "gemm4_kernel<64,128,plain>"),
    (77, 768, 768, True, True, "none", 1.0, "gemm4_kernel<64,64,plain>"),
    (77, 3072, 768, True, False, "quick_gelu", 1.0, "gemm4_kernel<64,128,plain>"),
    (77, 768, 3072, True, True, "none", 1.0, "gemm4_kernel<64,64,plain>+splitk_reduce_kernel"),
    (231, 2304, 768, True, False, "none", 1.0, "gemm4_kernel<64,128,plain>"),
    (231, 768, 768, True, True, "none", 1.0, "gemm4_kernel<64,64,plain>"),
    (231, 3072, 768, True, False, "quick_gelu", 1.0, "gemm4_kernel<64,128,plain>"),
    (231, 768, 3072, True, True, "none", 1.0, "gemm4_kernel<64,64,plain>+splitk_reduce_kernel"),
]


@pytest.mark.parametrize("M,N,K,bias,res,act,alpha,route", LINEAR_ROUTES, ids=lambda v: str(v))
def test_linear_route(ops, M, N, K, bias, res, act, alpha, route):
    """y = act(alpha x w^T + bias) + residual: route, then |y - y_hat| <= 2^-11 |y_hat| + L_act (c_acc(K) |alpha| |x||w|^T + 2^-23 |pre|)
    + 2^-23 |y_hat| (residual add) + 2^-24; GEGLU adds the GELU fit's 5.1e-7 |a| and its 5e-5 bias allowance."""
    x, w = r16((M, K), 11), r16((N, K), 12, 1 / math.sqrt(K))
    b = r16((N,), 13, 0.5) if bias else None
    n_out = N // 2 if act == "geglu" else N
    r = r16((M, n_out), 14) if res else None
    y = ops.linear(x, w, b, r, act=act, alpha=alpha)
    assert ops.last_kernel() == route
    ref, bound = EB.linear_ref(x, w, b, r, alpha, act)
    bm = int(route.split("<")[1].split(",")[0]) if route.startswith("gemm") and not route.startswith("gemm7") else 256
    EB.check(y, ref, bound, f"{route} {M}x{N}x{K} {act}", tile=(bm, 160), bias_extra=EB.GELU_FIT_BIAS if act == "geglu" else 0.0)
    rows = EB.boundary_rows(M, bm)
    cpu = EB.cpu_rows_linear(x, w, rows) * alpha
    if act != "geglu":
        dev = (x[rows].double() @ w.double().t()).cpu() * alpha
        assert torch.allclose(cpu, dev, rtol=1e-12, atol=1e-12)
        pre = cpu + (0.0 if b is None else b.double().cpu())
        yc = EB._act(pre, act) + (0.0 if r is None else r[rows].double().cpu())
        assert torch.allclose(yc, ref[rows].cpu(), rtol=1e-10, atol=1e-10)


def test_linear_route_independent_of_scratch_history(ops):
    """The split over K is capped by the scratch an op hands the kernels: a larger buffer cached by an earlier op (a convolution asks
    for 192 MB) must not change a later linear's route.  3968 x 2560 x 1280 splits in two only with more than 64 MB of scratch."""
    M, N, K = 3968, 2560, 1280
    x, w = r16((M, K), 15), r16((N, K), 16, 1 / math.sqrt(K))
    y0 = ops.linear(x, w)
    first = ops.last_kernel()
    wp = ops.repack_conv_weight(r16((64, 64, 3, 3), 17, 1 / 24))
    ops.conv2d(r16((1, 8, 8, 64), 18), wp, None)
    y1 = ops.linear(x, w)
    assert ops.last_kernel() == first == "gemm3_kernel<128,160,plain>"
    assert torch.equal(y0, y1)


def _ln_ref(x, w_prod, b_prod, gamma, beta, w, bias, t, eps, geglu):
    """fp64 LayerNorm(t) w^T + bias from the kernel's own fp16 t (the first GEMM is checked on its own), and the bound terms of the fold:
    gamma w rounded to fp16 once (2^-11 rstd |t| |gamma w|^T), the fp32 rstd (t W'^T - mu wsum) cancellation (c_acc + 2^-23 of each side)."""
    td = t.double()
    mu = td.mean(-1, keepdim=True)
    var = ((td - mu) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xn = (td - mu) * rstd * gamma.double() + beta.double()
    gw = (w.double() * gamma.double())
    acc = xn @ w.double().t()
    absdot = xn.abs() @ w.double().abs().t()
    side = rstd * (td.abs() @ gw.abs().t())
    extra = EB.U * side + EB.c_acc(t.shape[-1]) * side + 2.0 ** -23 * rstd * mu.abs() * gw.abs().sum(-1) + EB.U * (beta.double().abs() @ w.double().abs().t())
    bb = bias.double() if bias is not None else None
    return EB.epilogue_ref(acc, absdot, t.shape[-1], bb, None, 1.0, "geglu" if geglu else "none", extra=extra)


# (M, C, N, geglu, expected route: producer;consumer)
LN_ROUTES = [
    (512, 320, 320, False, "gemm4_kernel<64,64,plain>;gemm4_kernel<64,64,plain>"),
    (48897, 320, 320, False, "gemm7_kernel<256,K320,plain>;gemm7_kernel<256,K320,plain,ln>"),
    (48897, 320, 2560, True, "gemm7_kernel<256,K320,plain>;gemm7_kernel<256,K320,geglu,ln>"),
    (16384, 2560, 960, False, "gemm5_kernel<256,320,lnfold>;gemm5_kernel<256,320,lnfold>"),
    (4096, 640, 640, False, "gemm3_kernel<64,64,plain>;gemm3_kernel<64,64,plain>"),
]


@pytest.mark.parametrize("M,C,N,geglu,route", LN_ROUTES, ids=lambda v: str(v))
def test_linear_ln_route(ops, M, C, N, geglu, route):
    """The LayerNorm fold pair: t checked as a plain linear, y against fp64 LayerNorm(t) w^T + bias (see _ln_ref for the fold's terms)."""
    x, wp, bp = r16((M, C), 21), r16((C, C), 22, 1 / math.sqrt(C)), r16((C,), 23, 0.2)
    gamma, beta = r16((C,), 24, 0.2, 1.0), r16((C,), 25, 0.2)
    w, b = r16((N, C), 26, 1 / math.sqrt(C)), r16((N,), 27, 0.2)
    t, y = (ops.linear_ln_geglu if geglu else ops.linear_ln)(x, wp, bp, gamma, beta, w, b)
    assert ops.last_kernel() == route
    tref, tb = EB.linear_ref(x, wp, bp)
    EB.check(t, tref, tb, f"{route} producer {M}x{C}")
    ref, bound = _ln_ref(x, wp, bp, gamma, beta, w, b, t, 1e-5, geglu)
    EB.check(y, ref, bound, f"{route} consumer {M}x{C}x{N}", bias_extra=EB.GELU_FIT_BIAS if geglu else 0.0)


# ------------------------------------------------------------------ convolutions (ld_op_conv)

# (n, h, w, c1, c2, cout, stride, out_hw, ksize, rowvec, residual, expected route)
CONV_ROUTES = [
    # row-resident conv8: the one / two-image 8..64-pixel levels
    (2, 8, 8, 1280, 0, 1280, 1, None, 3, False, True, "conv8_kernel<W8>"),
    (2, 4, 4, 1280, 0, 1280, 1, (8, 8), 3, False, False, "conv8_kernel<W8,up>"),
    (2, 16, 16, 640, 0, 640, 1, None, 3, True, True, "conv8_kernel<W16>"),
    (2, 8, 8, 640, 0, 640, 1, (16, 16), 3, False, False, "conv8_kernel<W16,up>"),
    (2, 32, 32, 320, 0, 320, 1, None, 3, True, False, "conv8_kernel<W32>"),
    (2, 16, 16, 320, 0, 320, 1, (32, 32), 3, False, False, "conv8_kernel<W32,up>"),
    (2, 64, 64, 320, 0, 320, 1, None, 3, False, True, "conv8_kernel<W64>"),
    (1, 32, 32, 320, 0, 320, 1, (64, 64), 3, False, False, "conv8_kernel<W64,up>"),
    # halo-tile conv6: whole image rows per tile, >= 192 tiles (x split)
    (12, 64, 64, 320, 0, 320, 1, None, 3, True, True, "conv6_kernel<W64,halo>"),
    (12, 32, 32, 320, 0, 320, 1, (64, 64), 3, False, False, "conv6_kernel<W64,halo,up>"),
    (48, 32, 32, 320, 0, 320, 1, None, 3, False, False, "conv6_kernel<W32,halo>"),
    (192, 16, 16, 320, 0, 320, 1, None, 3, False, False, "conv6_kernel<W16,halo>"),
    (3, 128, 128, 256, 0, 256, 1, None, 3, False, True, "conv6_kernel<W128,halo,256>"),
    (3, 64, 64, 256, 0, 256, 1, (128, 128), 3, False, False, "conv6_kernel<W128,halo,256,up>"),
    (12, 64, 64, 256, 0, 256, 1, None, 3, False, False, "conv6_kernel<W64,halo,256>"),
    (2, 256, 256, 128, 0, 128, 1, None, 3, False, True, "conv6_kernel<W128,halo,128x512>"),
    (1, 512, 384, 128, 0, 32, 1, None, 3, False, False, "conv6_kernel<W128,halo,32x512>"),
    # implicit GEMM on the general tiles
    (48, 16, 16, 320, 0, 320, 1, (32, 32), 3, False, False, "conv6_kernel<W32,halo,up>"),
    (3, 64, 64, 320, 0, 320, 1, (128, 128), 3, False, True, "conv6_kernel<W128,halo,up>"),
    (16, 16, 16, 1280, 0, 1280, 1, None, 3, False, False, "conv6_kernel<W16,halo>+splitk_reduce_kernel"),
    (16, 8, 8, 1280, 0, 1280, 1, (16, 16), 3, False, False, "conv6_kernel<W16,halo,up>+splitk_reduce_kernel"),
    (8, 16, 16, 1280, 0, 1280, 1, (32, 32), 3, False, False, "conv6_kernel<W32,halo,up>+splitk_reduce_kernel"),
    # implicit GEMM on the general tiles
    (2, 33, 17, 64, 0, 320, 1, None, 3, True, True, "gemm3_kernel<64,160,conv>"),                    # 36 tiles, K / 640 < 2: no split
    (2, 8, 8, 64, 0, 320, 1, (33, 17), 3, False, False, "gemm3_kernel<64,160,conv>"),                # nearest, not 2x
    (1, 24, 24, 640, 0, 640, 1, None, 3, False, True, "gemm3_kernel<64,160,conv>+splitk_reduce_kernel"),
    (2, 11, 9, 320, 0, 320, 1, None, 3, True, True, "gemm3_kernel<64,160,conv,deep>+splitk_reduce_kernel"),   # <= 32 tiles
    (2, 8, 8, 320, 0, 320, 1, (11, 9), 3, False, False, "gemm3_kernel<64,160,conv,deep>+splitk_reduce_kernel"),
    (1, 17, 17, 640, 0, 320, 2, None, 3, False, False, "gemm3_kernel<64,160,conv,deep>+splitk_reduce_kernel"),  # stride 2 on odd sizes
    (1, 8, 8, 1280, 0, 1280, 1, None, 3, False, False, "gemm3_kernel<64,160,conv,deep>+splitk_reduce_kernel"),
    (16, 32, 32, 640, 0, 640, 1, None, 3, False, True, "gemm3_kernel<128,160,conv>"),
    (8, 16, 16, 1280, 0, 1280, 1, None, 3, True, False, "gemm3_kernel<128,160,conv>+splitk_reduce_kernel"),
    (2, 40, 40, 640, 640, 640, 1, None, 1, False, True, "gemm4_kernel<64,64,conv,2wg>"),              # 1x1 over two sources
    (2, 32, 32, 128, 64, 256, 1, None, 3, False, False, "gemm3_kernel<64,128,conv>+splitk_reduce_kernel"),
    (4, 64, 64, 512, 0, 512, 1, None, 3, False, True, "gemm3_kernel<128,128,conv>"),
    # H != W, the levels of a 512 x 768 request (latent 96 x 64): the halo tile with 24 / 12 four- and eight-row tiles per image, the smallest
    # image counts that keep 192 tiles
    (8, 96, 64, 320, 0, 320, 1, None, 3, True, True, "conv6_kernel<W64,halo>"),
    (8, 48, 32, 320, 0, 320, 1, (96, 64), 3, False, False, "conv6_kernel<W64,halo,up>"),
    (32, 48, 32, 320, 0, 320, 1, None, 3, False, True, "conv6_kernel<W32,halo>"),
    (32, 24, 16, 320, 0, 320, 1, (48, 32), 3, False, False, "conv6_kernel<W32,halo,up>"),
    (128, 24, 16, 320, 0, 320, 1, None, 3, False, False, "gemm5_kernel<256,320,conv>"),            # 24 rows are no whole 16-row W16 tiles: declined
    # the declines at full width: two portrait images per level (the row-resident kernel takes Ho == Wo only, the halo tile has too few tiles)
    # and a landscape level (a 96-pixel row is no tile width of either)
    (2, 12, 8, 1280, 0, 1280, 1, None, 3, False, True, "gemm3_kernel<64,160,conv,deep>+splitk_reduce_kernel"),
    (2, 24, 16, 640, 0, 640, 1, None, 3, True, False, "gemm3_kernel<64,160,conv>+splitk_reduce_kernel"),
    (2, 48, 32, 320, 0, 640, 1, None, 3, False, False, "gemm3_kernel<64,160,conv>+splitk_reduce_kernel"),
    (2, 64, 96, 320, 0, 320, 1, None, 3, True, True, "gemm3_kernel<64,160,conv,deep>"),
    (2, 96, 64, 320, 0, 320, 1, None, 3, False, False, "gemm3_kernel<64,160,conv,deep>"),
    # ControlNet's zero convolutions: ONE source, 1x1, C -> C, no residual, no row vector — every kernel the launch tables of
    # tests/test_controlnet_chain_gpu.py / _full_gpu.py show for them, each at the smallest problem gemm_plan still gives that kernel
    # (gemm.hip: the v3 / v4 tail; tiles = ceil(M / bm) * ceil(N / 160)):
    (2, 2, 2, 1280, 0, 1280, 1, None, 1, False, False, "gemm3_kernel<64,160,conv,deep>+splitk_reduce_kernel"),   # the 2 x 2 level of a 16 x 16 latent: 8 rows; K / 640 = 2 slices
    (1, 1, 1, 320, 0, 320, 1, None, 1, False, False, "gemm3_kernel<64,160,conv,deep>"),              # <= 32 tiles, K < 1280: no split; one row
    (1, 45, 45, 1280, 0, 1280, 1, None, 1, False, False, "gemm3_kernel<64,160,conv,deep>"),          # 32 panels x 8 = 256 tiles: the low edge of deep's one round (2025 rows, a ragged last panel; 26 panels up: past skinny_conv1)
    (1, 19, 27, 640, 0, 640, 1, None, 1, False, False, "gemm3_kernel<64,160,conv>"),                 # 513 rows: 9 panels x 4 = 36 tiles, the first count above deep's 32
    (1, 89, 91, 1280, 0, 1280, 1, None, 1, False, False, "gemm3_kernel<128,160,conv>"),              # 8099 rows: 64 panels of 128 x 8 = 512 tiles, where bm turns 128 (8064 rows: still 63)
    (1, 5, 77, 1280, 0, 1280, 1, None, 1, False, False, "gemm4_kernel<64,64,conv,2wg>"),             # skinny_conv1: 385 rows = 7 x 20 = 140 tiles of 64 x 64 > 128, 1280 <= K <= 3200
    (1, 1, 2, 256, 0, 256, 1, None, 1, False, False, "gemm3_kernel<64,128,conv>"),                   # the tiny configuration's (N = 64 / 128 / 256 takes 128 columns): its 1 x 2 level
]


@pytest.mark.parametrize("n,h,w,c1,c2,cout,stride,out_hw,ksize,rv,res,route", CONV_ROUTES, ids=lambda v: str(v))
def test_conv_route(ops, n, h, w, c1, c2, cout, stride, out_hw, ksize, rv, res, route):
    """NHWC convolution against fp64 im2col + matmul on the device and a CPU fp64 patch sum at the image corners, band edges and tile
    boundaries; bound as for a linear with K = C k^2 (2^-11 |y_hat| + c_acc(K) |cols| |W|^T + 2^-23 per epilogue add + 2^-24)."""
    x = r16((n, h, w, c1), 31)
    x2 = r16((n, h, w, c2), 32) if c2 else None
    wt = r16((cout, c1 + c2, ksize, ksize), 33, 1 / math.sqrt(ksize * ksize * (c1 + c2)))
    b = r16((cout,), 34, 0.5)
    rowvec = r16((n, cout), 35, 0.5) if rv else None
    hv, wv = (h, w) if out_hw is None else out_hw
    ho, wo = ((hv - 1) // stride + 1, (wv - 1) // stride + 1) if ksize == 3 else (hv, wv)
    resid = r16((n, ho, wo, cout), 36) if res else None
    wp = ops.repack_conv_weight(wt)
    y = ops.conv2d(x, wp, b, ksize, stride, x2=x2, out_hw=out_hw, rowvec=rowvec, residual=resid)
    assert ops.last_kernel() == route
    ref, bound, _ = EB.conv_ref(x, wt, b, resid, stride, out_hw, x2, rowvec)
    y2 = y.reshape(-1, cout)
    EB.check(y2, ref, bound, f"{route} n{n} {h}x{w} c{c1}+{c2}->{cout}", image_rows=ho * wo, width=wo)
    rows = EB.boundary_rows(y2.shape[0], 256, ho * wo, wo)
    cpu = EB.cpu_rows_conv(x, wt, rows, stride, out_hw, x2)
    dev = (EB.im2col(x if x2 is None else torch.cat([x, x2], -1), ksize, stride, out_hw)[rows] @ wt.double().reshape(cout, -1).t()).cpu()
    assert torch.allclose(cpu, dev, rtol=1e-10, atol=1e-10)


# (n, h, w, c1, c2, cout, expected route): GroupNorm(32) + SiLU fused into the halo tile's loader; c1 = 128 / c2 = 192 puts groups of 10
# channels across the two sources' boundary
GN_CONV_ROUTES = [
    (12, 64, 64, 320, 0, 320, "conv6_kernel<W64,halo+groupnorm>"),
    (12, 64, 64, 128, 192, 320, "conv6_kernel<W64,halo+groupnorm>"),
    (3, 128, 128, 256, 0, 256, "conv6_kernel<W128,halo+groupnorm,256>"),
    (2, 256, 256, 128, 0, 128, "conv6_kernel<W128,halo+groupnorm,128x512>"),
    (3, 128, 128, 320, 0, 320, "conv6_kernel<W128,halo+groupnorm>"),
    # H != W: level 0 of a 512 x 768 request, 24 four-row tiles per image, 192 in all
    (8, 96, 64, 320, 0, 320, "conv6_kernel<W64,halo+groupnorm>"),
    (8, 96, 64, 128, 192, 320, "conv6_kernel<W64,halo+groupnorm>"),
    (2, 64, 96, 320, 0, 320, "gemm3_kernel<64,160,conv,deep>"),           # landscape: the two-pass GroupNorm in front of the general tiles
]


@pytest.mark.parametrize("n,h,w,c1,c2,cout,route", GN_CONV_ROUTES, ids=lambda v: str(v))
def test_groupnorm_conv_route(ops, n, h, w, c1, c2, cout, route):
    """conv3x3(SiLU(GroupNorm32(cat(x1, x2)))) + bias against errbound.gn_silu_conv_ref: the loader rounds the normalised, activated operand to fp16
    once, and the operand's error — that rounding and the fp32 statistics' share, cancellation term included — comes from groupnorm_ref's model
    and reaches the output as im2col(e_a) |W|^T (tests/test_adverse_routes_gpu.py runs the same rows where the statistics' share is visible)."""
    C = c1 + c2
    x = r16((n, h, w, c1), 41, 1.0, 0.3)
    x2 = r16((n, h, w, c2), 42, 2.0, -0.5) if c2 else None
    gamma, beta = r16((C,), 43, 0.2, 1.0), r16((C,), 44, 0.2)
    wt = r16((cout, C, 3, 3), 45, 1 / math.sqrt(9 * C))
    b = r16((cout,), 46, 0.5)
    y = ops.group_norm_silu_conv2d(x, gamma, beta, 1e-5, ops.repack_conv_weight(wt), b, x2=x2)
    assert ops.last_kernel().endswith(route)
    ref, bound = EB.gn_silu_conv_ref(x, gamma, beta, 1e-5, wt, b, x2=x2)
    EB.check(y.reshape(-1, cout), ref, bound, f"{route} n{n} {h}x{w} c{c1}+{c2}->{cout}", image_rows=h * w, width=w)


# (n, h, w, c, cout, expected route): 3x3 convolutions that also hand the next GroupNorm its partial statistics (ld_op_conv_gn_partials)
GN_PART_ROUTES = [
    (1, 8, 8, 1280, 1280, "gemm3_kernel<64,160,conv,deep>+splitk_reduce_gn_kernel"),
    (1, 24, 24, 640, 640, "gemm3_kernel<64,160,conv>+splitk_reduce_gn_kernel"),
    (8, 16, 16, 1280, 1280, "gemm3_kernel<128,160,conv>+splitk_reduce_gn_kernel"),
    (8, 32, 32, 1280, 640, "conv6_kernel<W32,halo>+splitk_reduce_gn_kernel"),
    (16, 16, 16, 1280, 1280, "conv6_kernel<W16,halo>+splitk_reduce_gn_kernel"),
    (8, 48, 32, 1280, 640, "conv6_kernel<W32,halo>+splitk_reduce_gn_kernel"),          # H != W: level 1 of a 512 x 768 request
    (8, 24, 16, 1280, 1280, "gemm3_kernel<128,160,conv>+splitk_reduce_gn_kernel"),     # its level 2: no whole W16 tiles
]


SKIP_ROUTES = [
    (12, 64, 64, 320, 320, 320, 320, "gemm5_kernel<256,320,conv>"),        # 192 tiles of 256 x 320, K = 9 c + skip channels
    (8, 96, 64, 320, 320, 320, 320, "gemm5_kernel<256,320,conv>"),         # H != W: 192 tiles of four image rows
]


@pytest.mark.parametrize("n,h,w,c,sc1,sc2,cout,route", SKIP_ROUTES, ids=lambda v: str(v))
def test_conv_skip_route(ops, n, h, w, c, sc1, sc2, cout, route):
    """ResBlock's out-conv + 1x1 skip as one contraction: the reference appends the skip sources to the im2col columns (same bound)."""
    x, s1, s2 = r16((n, h, w, c), 61), r16((n, h, w, sc1), 62), r16((n, h, w, sc2), 63)
    wt = r16((cout, c, 3, 3), 64, 1 / math.sqrt(9 * c + sc1 + sc2))
    wsk = r16((cout, sc1 + sc2), 65, 1 / math.sqrt(9 * c + sc1 + sc2))
    b, bsk = r16((cout,), 66, 0.5), r16((cout,), 67, 0.5)
    y = ops.conv2d_skip(x, ops.repack_conv_weight(wt), b, s1, s2, wsk, bsk)
    assert ops.last_kernel() == route
    cols = torch.cat([EB.im2col(x, 3), torch.cat([s1, s2], -1).double().reshape(-1, sc1 + sc2)], 1)
    wm = torch.cat([wt.double().reshape(cout, -1), wsk.double()], 1)
    ref, bound = EB.epilogue_ref(cols @ wm.t(), cols.abs() @ wm.abs().t(), wm.shape[1], b.double() + bsk.double())
    EB.check(y.reshape(-1, cout), ref, bound, f"{route} n{n} {h}x{w}", image_rows=h * w, width=w, tile=(256, 320))



@pytest.mark.parametrize("n,h,w,c,cout,route", GN_PART_ROUTES, ids=lambda v: str(v))
def test_conv_gn_partials_route(ops, n, h, w, c, cout, route):
    """The convolution's own bound (as test_conv_route), then the partial statistics against fp64 sums of the STORED fp16 outputs: the
    reduce pass adds fp32 values of magnitude |y|, so sum and sum of squares carry c_acc(HW) of the sums of |y| and y^2."""
    x = r16((n, h, w, c), 51)
    wt = r16((cout, c, 3, 3), 52, 1 / math.sqrt(9 * c))
    b = r16((cout,), 53, 0.5)
    y, part = ops.conv2d_gn_partials(x, ops.repack_conv_weight(wt), b)
    assert ops.last_kernel() == route
    ref, bound, _ = EB.conv_ref(x, wt, b)
    EB.check(y.reshape(-1, cout), ref, bound, f"{route} n{n} {h}x{w} c{c}->{cout}", image_rows=h * w, width=w)
    assert part is not None
    yg = y.double().view(n, h * w, 32, cout // 32)
    got = part.double().sum(1)
    want = torch.stack([yg.sum((1, 3)), (yg * yg).sum((1, 3))], -1)
    tol = torch.stack([yg.abs().sum((1, 3)), (yg * yg).sum((1, 3))], -1) * (EB.c_acc(h * w * cout // 32) + 2.0 ** -22) + EB.TINY
    assert bool(((got - want).abs() <= tol).all()), float(((got - want).abs() / tol).max())


# ------------------------------------------------------------------ completeness against the profiled forwards

def route_names():
    """Every instantiation name the tables above pin (a route string may hold several, joined by ';' and '+')."""
    names = set()
    for table, col in ((ATTN_ROUTES, -1), (LINEAR_ROUTES, -1), (LN_ROUTES, -1), (CONV_ROUTES, -1), (GN_CONV_ROUTES, -1), (GN_PART_ROUTES, -1), (SKIP_ROUTES, -1)):
        for row in table:
            for part in row[col].split(";"):
                names.add(part)
                names.update(part.split("+"))
    return names


def _contraction(name):
    return any(name.startswith(b) for b in ("gemm", "conv6_kernel", "conv8_kernel", "flash_attn", "splitk_reduce"))


def halo_routes_off_square():
    """The routes of the convolution tables' rows with H != W (the size the kernel runs at: out_hw where the row resizes)."""
    routes = set()
    for table, hw_of in ((CONV_ROUTES, lambda r: r[7] or (r[1], r[2])), (GN_CONV_ROUTES, lambda r: (r[1], r[2])), (GN_PART_ROUTES, lambda r: (r[1], r[2])),
                         (SKIP_ROUTES, lambda r: (r[1], r[2]))):
        routes.update(row[-1] for row in table if hw_of(row)[0] != hw_of(row)[1])
    return routes


@pytest.mark.parametrize("batch,hw,pair", [(8, (64, 64), True), (1, (64, 64), True), (4, (128, 128), True), (4, (96, 64), True), (1, (64, 96), True)],
                         ids=lambda v: (str(v[0]) if v[0] == v[1] else f"{v[0]}x{v[1]}") if isinstance(v, tuple) else None)
def test_unet_forward_routes_are_pinned(batch, hw, pair):
    """Every contraction instantiation the profiled SD1.5 UNet forward (CFG pair) dispatches at batch 8 / 1 at 64^2, at the hires step
    (b = 4 at 128^2) and at the non-square requests (b = 4 at 96 x 64, b = 1 at 64 x 96) has a row above, with its epilogue / split suffix.
    The name alone does not say at which geometry a row runs: every halo-tile route a NON-SQUARE forward dispatches also has a row with
    H != W (tiles of whole image rows: the tile count per image and the band edges follow H, the tile width W)."""
    from lightdiffusion_amd import weights as W
    from lightdiffusion_amd.unet import synthetic_unet
    h, w = hw
    u = synthetic_unet(W.sd15_unet_config(), max_batch=2 * batch, max_hw=(h, w))
    u.set_context(torch.randn(2 * batch, 77, 768))
    x = torch.randn(batch, 4, h, w, device=DEV)
    u.profile_pair(x, torch.full((batch,), 3.0, device=DEV))
    seen = {k for k in u.profile_kernels() if _contraction(k)}
    assert seen, "no contraction kernels profiled"
    missing = sorted(seen - route_names())
    assert not missing, f"dispatched but not pinned by a route row: {missing}"
    if h != w:
        halo = {k for k in seen if k.startswith("conv6_kernel<") and "halo" in k}
        # (portrait: 64-, 32- and 16-pixel rows are tile widths; landscape: 96-, 48- and 24-pixel rows are not)
        assert bool(halo) == (w == 64), f"{batch} x {h} x {w}: halo-tile routes {sorted(halo)}"
        square_only = sorted(halo - halo_routes_off_square())
        assert not square_only, f"halo-tile routes of a non-square forward whose rows are all square: {square_only}"


def test_vae_decode_routes_are_pinned():
    """The same for the VAE decode at 512^2, batch 8."""
    from lightdiffusion_amd import weights as W
    from lightdiffusion_amd.unet import synthetic_vae
    v = synthetic_vae(W.sd15_vae_config(), max_batch=8, max_hw=(64, 64))
    rows = v.profile_decode(torch.randn(8, 4, 64, 64))
    seen = {r[-1] for r in rows if _contraction(r[-1])}
    assert seen
    missing = sorted(seen - route_names())
    assert not missing, f"dispatched but not pinned by a route row: {missing}"


def test_clip_forward_routes_are_pinned():
    """The same for the text model, whose operator calls come from Python (CLIPTextModelHIP._encode): every contraction the recorder of
    tests/clip_chain.py sees at CLIP-L's width with B = 1, 2, 3 prompts (M = 77, 154, 231) has a row above."""
    import clip_chain as C
    from lightdiffusion_amd import ops as o
    from lightdiffusion_amd.clip import CLIPTextModelHIP
    cfg = C.config("w2")
    tm = CLIPTextModelHIP(cfg, C.state_dict(cfg), device=DEV)
    seen = set()
    for B in (1, 2, 3):
        calls, _ = C.run(o, tm, C.prompts(B))
        for c in calls:
            for part in c["launches"].split(";"):
                seen.update(k for k in [part] + part.split("+") if _contraction(k))
    assert any(k.startswith("gemm") for k in seen) and any(k.startswith("flash_attn") for k in seen), seen
    missing = sorted(seen - route_names())
    assert not missing, f"dispatched but not pinned by a route row: {missing}"
