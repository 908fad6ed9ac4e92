"""GPU: the memory footprint of every pinned route, and the executors' independence of their workspace's history.

tests/test_routes_gpu.py holds the VALUES of every contraction, attention and norm route to fp64 on exact-size torch tensors.  This module runs
the same rows (same tables, same seeds, same scratch sizes, through the C ABI) three times each by tests/footprint.py: plain; with every operand
inside a buffer of its own whose guards and pitch gaps hold NaN, the outputs NaN inside 0xAAAA guards and the scratch 0xFF bytes inside guards;
and again with +Inf and a zeroed scratch.  Per guarded run: the same route, every output bit-identical to the plain run, every output element
written, every guard, gap and scratch guard intact.  No tolerance and no reference: the plain call is the one the route tests hold to fp64.

Pitches where the ABI has them: attention q / k / v / o at H d + 8 (the batch stride is lq * ld in the ABI, so there is no gap between batch
elements to poison), the q|k|v seam at 3C, ld_op_linear_batched with lda, ldw and all three batch strides one row longer than minimal and
n_valid < N (the three contractions of the VAE's AttnBlock at the fallback width 64), ld_op_conv under LD_FORM_VAE with n_valid = ldc = 8 on
weights whose rows 8 .. 31 are NaN.  A transposed V keeps its zero key padding Lk .. round8(Lk): the header makes that the caller's duty.

The history tests run each resident model (tiny configs, tests/test_lifecycle_gpu.py's families) on two identical handles reserved at the larger
shape: handle 1 sees the large shape on adverse inputs first, then the small odd one; handle 2 only the small one; then handle 1 the small one
again.  All three small results are the same bits.
"""
import ctypes as C
import math

import pytest
import torch

import adverse as A
import footprint as FP
import test_routes_gpu as R
from test_lifecycle_gpu import FAMILIES, load, make      # noqa: F401  (make: the fixture, used by name)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
r16 = R.r16
ids = lambda v: str(v)      # noqa: E731


@pytest.fixture(scope="module")
def L():
    from lightdiffusion_amd._lib import lib
    return lib()


@pytest.fixture(scope="module")
def ops(L):
    from lightdiffusion_amd import ops as o
    return o


_SCRATCH = FP.Scratch(DEV)


def stream():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


def ok(L, st, where):
    from lightdiffusion_amd._lib import check
    check(st, where)
    return L.ld_op_last_kernel().decode()


def hold(ops, call, inputs, outputs, ws_bytes=0, expect=None, what=""):
    """footprint.hold with the plain run's scratch the one the ops wrappers hand out, and the module's guarded scratch."""
    inputs = {k: v for k, v in inputs.items() if v is not None}
    return FP.hold(call, inputs, outputs, ws_bytes, expect, what, scratch=_SCRATCH, plain_scratch=lambda n: ops._ws(n, DEV))


H16 = torch.float16
F32 = torch.float32


# ------------------------------------------------------------------ attention

def _attention(L, ops, seam, b, heads, lq, lk, d, causal, route, q, k, v):
    c = heads * d
    scale = 1.0 / math.sqrt(d)
    gap = dict(pitch=c + 8)
    if seam == "qkv":
        qkv = torch.cat([q, k, v], -1).contiguous()

        def call(I, O, ws):
            t, o = I["qkv"], O["o"]
            base = t.data_ptr()
            return ok(L, L.ld_op_attention_rowv(base, t.stride(1), base + 2 * c, t.stride(1), base + 4 * c, t.stride(1), ptr(o), o.stride(1), b, heads, lq, lk, d,
                                                scale, int(causal), stream()), "ld_op_attention_rowv")
        inputs = {"qkv": qkv}                      # the seam's pitch is 3C: q, k and v are each other's pitch gaps
    elif seam == "rowv":
        def call(I, O, ws):
            qq, kk, vv, o = I["q"], I["k"], I["v"], O["o"]
            return ok(L, L.ld_op_attention_rowv(ptr(qq), qq.stride(1), ptr(kk), kk.stride(1), ptr(vv), vv.stride(1), ptr(o), o.stride(1), b, heads, lq, lk, d,
                                                scale, int(causal), stream()), "ld_op_attention_rowv")
        inputs = {"q": (q, gap), "k": (k, gap), "v": (v, gap)}
    else:
        lkp = (lk + 7) // 8 * 8
        vt = torch.zeros(b, c, lkp, dtype=H16, device=DEV)     # the key padding lk .. lkp stays zero: the caller's duty (include/ld_mi355x.h)
        vt[:, :, :lk] = v.transpose(1, 2)

        def call(I, O, ws):
            qq, kk, tt, o = I["q"], I["k"], I["vt"], O["o"]
            return ok(L, L.ld_op_attention(ptr(qq), qq.stride(1), ptr(kk), kk.stride(1), ptr(tt), tt.stride(1), ptr(o), o.stride(1), b, heads, lq, lk, d, scale,
                                           int(causal), stream()), "ld_op_attention")
        inputs = {"q": (q, gap), "k": (k, gap), "vt": vt}
    hold(ops, call, inputs, {"o": ((b, lq, c), H16, gap)}, 0, route, f"attention {seam} b{b} h{heads} Lq{lq} Lk{lk} d{d}")


@pytest.mark.parametrize("rowv,b,heads,lq,lk,d,causal,route", R.ATTN_ROUTES, ids=ids)
def test_attention_footprint(L, ops, rowv, b, heads, lq, lk, d, causal, route):
    """Q rows >= Lq, K / V rows >= Lk, the columns behind H d of every row and d's tail inside its k-step are poison; O at a pitch of H d + 8."""
    q, k, v = r16((b, lq, heads * d), 1), r16((b, lk, heads * d), 2), r16((b, lk, heads * d), 3)
    _attention(L, ops, "rowv" if rowv else "vt", b, heads, lq, lk, d, causal, route, q, k, v)


QKV_SEAM = [row[:8] for row in R.ATTN_PEAKED if row[0] == "qkv"]


@pytest.mark.parametrize("seam,b,heads,lq,lk,d,causal,route", QKV_SEAM, ids=ids)
def test_attention_qkv_seam_footprint(L, ops, seam, b, heads, lq, lk, d, causal, route):
    """The executors' own layout: q, k, v column blocks of one [b][L][3C] tensor."""
    q, k, v = r16((b, lq, heads * d), 1), r16((b, lk, heads * d), 2), r16((b, lk, heads * d), 3)
    _attention(L, ops, seam, b, heads, lq, lk, d, causal, route, q, k, v)


# ------------------------------------------------------------------ linear

ACT = {"none": 0, "silu": 1, "geglu": 2, "quick_gelu": 3}


@pytest.mark.parametrize("M,N,K,bias,res,act,alpha,route", R.LINEAR_ROUTES, ids=ids)
def test_linear_footprint(L, ops, M, N, K, bias, res, act, alpha, route):
    """ld_op_linear under the wrapper's 64 MB of scratch: M ragged against the tile, K % 64 in {8, 24, 56}, the split-K slabs and the GEGLU repack."""
    n_out = N // 2 if act == "geglu" else N
    inputs = {"x": r16((M, K), 11), "w": r16((N, K), 12, 1 / math.sqrt(K)), "b": r16((N,), 13, 0.5) if bias else None,
              "r": r16((M, n_out), 14) if res else None}

    def call(I, O, ws):
        return ok(L, L.ld_op_linear(ptr(I["x"]), ptr(I["w"]), ptr(I.get("b")), ptr(I.get("r")), ptr(O["y"]), M, N, K, alpha, ACT[act], ptr(ws), ws.numel(),
                                    stream()), "ld_op_linear")
    hold(ops, call, inputs, {"y": ((M, n_out), H16)}, 64 << 20, route, f"linear {M}x{N}x{K} {act}")


@pytest.mark.parametrize("M,C,N,geglu,route", R.LN_ROUTES, ids=ids)
def test_linear_ln_footprint(L, ops, M, C, N, geglu, route):
    """The LayerNorm fold pair: both outputs, t and y, and the fold's temporaries in the scratch."""
    inputs = {"x": r16((M, C), 21), "wp": r16((C, C), 22, 1 / math.sqrt(C)), "bp": r16((C,), 23, 0.2), "gamma": r16((C,), 24, 0.2, 1.0),
              "beta": r16((C,), 25, 0.2), "w": r16((N, C), 26, 1 / math.sqrt(C)), "b": r16((N,), 27, 0.2)}
    fn = L.ld_op_linear_ln_geglu if geglu else L.ld_op_linear_ln
    nbytes = ((4 * N * C + 12 * N) if geglu else (2 * N * C + 8 * N)) + 8 * ((C + 63) // 64) * M + 4096

    def call(I, O, ws):
        return ok(L, fn(ptr(I["x"]), ptr(I["wp"]), ptr(I["bp"]), None, ptr(I["gamma"]), ptr(I["beta"]), ptr(I["w"]), ptr(I["b"]), ptr(O["t"]), ptr(O["y"]), M, C, N,
                        1e-5, ptr(ws), ws.numel(), stream()), "ld_op_linear_ln")
    hold(ops, call, inputs, {"t": ((M, C), H16), "y": ((M, N // 2 if geglu else N), H16)}, nbytes, route, f"linear_ln {M}x{C}x{N}")


# (latent h, w, batch) of tests/test_configs_gpu.py::test_vae_fallback_attention at its width C = 64: L = 35 / Lp = 40, and L = 9 / Lp = 16 at batch 2
BATCHED = [(which, hw, n) for hw, n in (((5, 7), 1), ((3, 3), 2)) for which in ("v^T", "qk^T", "pv")]


@pytest.mark.parametrize("which,hw,n", BATCHED, ids=ids)
def test_linear_batched_footprint(L, ops, which, hw, n):
    """The three contractions of the VAE's AttnBlock (tests/vae_chain.py) with row pitches 8 elements wider and batch strides one row longer than
    minimal; rows n_valid .. N-1 of w lie in the gap or the guard and are NaN / Inf, not zeros."""
    Cw, Lv = 64, hw[0] * hw[1]
    Lp = (Lv + 7) // 8 * 8
    wide = lambda rows, cols: dict(pitch=cols + 8, batch_stride=(rows + 1) * (cols + 8))      # noqa: E731
    if which == "v^T":       # V^T[b] = Wv g_b^T + bv along the rows: x shared (sA = 0), keys Lv .. Lp-1 of g do not exist
        M, N, K, nv, alpha = Cw, Lp, Cw, Lv, 1.0
        inputs = {"x": (r16((Cw, Cw), 71, 1 / 8), dict(pitch=Cw + 8)), "w": (r16((n, Lv, Cw), 72), wide(Lv, Cw)), "bias_m": r16((Cw,), 73, 0.5)}
    elif which == "qk^T":    # S_b = Q_b K_b^T / sqrt(C): x and w column blocks of one [n][L][2C] tensor
        M, N, K, nv, alpha = Lv, Lp, Cw, Lv, 1.0 / math.sqrt(Cw)
        inputs = {"qk": (r16((n, Lv, 2 * Cw), 74), wide(Lv, 2 * Cw))}
    else:                    # O_b = P_b V_b: K = Lp, a tail of the 64-wide k-step
        M, N, K, nv, alpha = Lv, Cw, Lp, 0, 1.0
        inputs = {"x": (r16((n, Lv, Lp), 75, 0.1), wide(Lv, Lp)), "w": (r16((n, Cw, Lp), 76), wide(Cw, Lp))}

    def call(I, O, ws):
        y = O["y"]
        if which == "qk^T":
            t = I["qk"]
            x, lda, w, ldw, sa, sw = t.data_ptr(), t.stride(1), t.data_ptr() + 2 * Cw, t.stride(1), t.stride(0), t.stride(0)
        else:
            x, w = I["x"], I["w"]
            lda, ldw, sa, sw = x.stride(-2), w.stride(1), (0 if x.dim() == 2 else x.stride(0)), w.stride(0)
            x, w = x.data_ptr(), w.data_ptr()
        return ok(L, L.ld_op_linear_batched(x, lda, w, ldw, None, ptr(I.get("bias_m")), ptr(y), M, N, K, nv, alpha, n, sa, sw, y.stride(0), ptr(ws), ws.numel(),
                                            stream()), "ld_op_linear_batched")
    route, _ = hold(ops, call, inputs, {"y": ((n, M, N), H16, dict(batch_stride=(M + 1) * N))}, 96 << 20, None, f"linear_batched {which} {hw} n{n}")
    assert route.startswith("gemm"), route


# ------------------------------------------------------------------ convolutions

def _conv_operands(n, h, w, c1, c2, cout, ksize, rv, res, ho, wo, ops):
    wt = r16((cout, c1 + c2, ksize, ksize), 33, 1 / math.sqrt(ksize * ksize * (c1 + c2)))
    return {"x": r16((n, h, w, c1), 31), "x2": r16((n, h, w, c2), 32) if c2 else None, "wt": ops.repack_conv_weight(wt), "b": r16((cout,), 34, 0.5),
            "rowvec": r16((n, cout), 35, 0.5) if rv else None, "r": r16((n, ho, wo, cout), 36) if res else None}


@pytest.mark.parametrize("n,h,w,c1,c2,cout,stride,out_hw,ksize,rv,res,route", R.CONV_ROUTES, ids=ids)
def test_conv_footprint(L, ops, n, h, w, c1, c2, cout, stride, out_hw, ksize, rv, res, route):
    """ld_op_conv under the wrapper's 192 MB: the image's border taps, M ragged against the tile, the split-K slabs, conv8's counters and weight copy."""
    hv, wv = (h, w) if out_hw is None else out_hw
    ho, wo = ((hv - 1) // stride + 1, (wv - 1) // stride + 1) if ksize == 3 else (hv, wv)
    inputs = _conv_operands(n, h, w, c1, c2, cout, ksize, rv, res, ho, wo, ops)

    def call(I, O, ws):
        return ok(L, L.ld_op_conv(ptr(I["x"]), c1, ptr(I.get("x2")), c2, n, h, w, hv, wv, stride, ksize, ptr(I["wt"]), ptr(I["b"]), ptr(I.get("rowvec")),
                                  ptr(I.get("r")), ptr(O["y"]), cout, -1, 0, 0, 0, 0, ops.FORM_UNET, ptr(ws), ws.numel(), stream()), "ld_op_conv")
    hold(ops, call, inputs, {"y": ((n, ho, wo, cout), H16)}, 192 << 20, route, f"conv n{n} {h}x{w} c{c1}+{c2}->{cout}")


VAE_OUT = [row for row in R.CONV_ROUTES if row[-1] == "conv6_kernel<W128,halo,32x512>"]


@pytest.mark.parametrize("n,h,w,c1,c2,cout,stride,out_hw,ksize,rv,res,route", VAE_OUT, ids=ids)
def test_conv_vae_out_footprint(L, ops, n, h, w, c1, c2, cout, stride, out_hw, ksize, rv, res, route):
    """The VAE's output convolution: LD_FORM_VAE, n_valid = ldc = 8 on weights of 32 rows whose rows 8 .. 31 hold NaN / Inf ("the others count
    as zeros"), 8 stored columns."""
    assert (cout, ksize, stride, c2) == (32, 3, 1, 0)
    inputs = _conv_operands(n, h, w, c1, 0, cout, 3, False, False, h, w, ops)
    for poison in ("nan", "inf"):
        wt = inputs["wt"].clone()
        wt[8:] = float(poison)
        ins = dict(inputs, wt=wt)

        def call(I, O, ws):
            return ok(L, L.ld_op_conv(ptr(I["x"]), c1, None, 0, n, h, w, h, w, 1, 3, ptr(I["wt"]), ptr(I["b"]), None, None, ptr(O["y"]), cout, -1, 0, 0, 8, 8,
                                      ops.FORM_VAE, ptr(ws), ws.numel(), stream()), "ld_op_conv")
        _, plain = hold(ops, call, ins, {"y": ((n, h, w, 8), H16)}, ops._VAE_WS, route, f"vae conv_out {poison} rows n{n} {h}x{w}")
        clean = ops.conv2d(inputs["x"], inputs["wt"][:8].contiguous().repeat(4, 1), inputs["b"], n_valid=8, ldc=8, form=ops.FORM_VAE)
        assert torch.equal(plain["y"].view(torch.int16), clean.view(torch.int16)), f"weight rows 8 .. 31 ({poison}) reached the stored columns"


@pytest.mark.parametrize("n,h,w,c1,c2,cout,route", R.GN_CONV_ROUTES, ids=ids)
def test_groupnorm_conv_footprint(L, ops, n, h, w, c1, c2, cout, route):
    """ld_op_groupnorm_conv: the statistics, scale / shift and the normalised tensor live in the scratch in front of the split partials."""
    C_ = c1 + c2
    inputs = {"x": r16((n, h, w, c1), 41, 1.0, 0.3), "x2": r16((n, h, w, c2), 42, 2.0, -0.5) if c2 else None, "gamma": r16((C_,), 43, 0.2, 1.0),
              "beta": r16((C_,), 44, 0.2), "wt": ops.repack_conv_weight(r16((cout, C_, 3, 3), 45, 1 / math.sqrt(9 * C_))), "b": r16((cout,), 46, 0.5)}

    def call(I, O, ws):
        return ok(L, L.ld_op_groupnorm_conv(ptr(I["x"]), c1, ptr(I.get("x2")), c2, n, h, w, ptr(I["gamma"]), ptr(I["beta"]), 1e-5, ptr(I["wt"]), ptr(I["b"]), None,
                                            None, ptr(O["y"]), cout, None, 0, None, None, ops.FORM_UNET, ptr(ws), ws.numel(), stream()), "ld_op_groupnorm_conv")
    hold(ops, call, inputs, {"y": ((n, h, w, cout), H16)}, L.ld_op_groupnorm_conv_ws_bytes(c1, c2, n, h, w, cout), lambda r: r.endswith(route),
         f"groupnorm_conv n{n} {h}x{w} c{c1}+{c2}->{cout}")


@pytest.mark.parametrize("n,h,w,c,cout,route", R.GN_PART_ROUTES, ids=ids)
def test_conv_gn_partials_footprint(L, ops, n, h, w, c, cout, route):
    """The secondary output: of the ld_op_conv_gn_partials_floats floats of `part` exactly [n][*chunks][32][2] are written, all of them, and
    nothing behind."""
    inputs = {"x": r16((n, h, w, c), 51), "wt": ops.repack_conv_weight(r16((cout, c, 3, 3), 52, 1 / math.sqrt(9 * c))), "b": r16((cout,), 53, 0.5)}
    floats = L.ld_op_conv_gn_partials_floats(n, h * w)
    seen = []

    def call(I, O, ws):
        chunks = C.c_int(-1)
        r = ok(L, L.ld_op_conv_gn_partials(ptr(I["x"]), c, None, 0, n, h, w, h, w, 1, 3, ptr(I["wt"]), ptr(I["b"]), None, ptr(O["y"]), cout, -1, 0, 0, 0, 0,
                                           ops.FORM_UNET, ptr(O["part"]), C.byref(chunks), ptr(ws), ws.numel(), stream()), "ld_op_conv_gn_partials")
        seen.append(chunks.value)
        return r
    outputs = {"y": ((n, h, w, cout), H16), "part": ((floats,), F32, dict(rows_behind=0, upto=lambda r: n * seen[-1] * 64))}
    hold(ops, call, inputs, outputs, 192 << 20, route, f"conv_gn_partials n{n} {h}x{w} c{c}->{cout}")
    assert len(set(seen)) == 1 and 0 < n * seen[0] * 64 <= floats, seen


@pytest.mark.parametrize("n,h,w,c,sc1,sc2,cout,route", R.SKIP_ROUTES, ids=ids)
def test_conv_skip_footprint(L, ops, n, h, w, c, sc1, sc2, cout, route):
    """ld_op_conv_skip: the folded weights and bias are built in the scratch first."""
    s = 1 / math.sqrt(9 * c + sc1 + sc2)
    inputs = {"x": r16((n, h, w, c), 61), "s1": r16((n, h, w, sc1), 62), "s2": r16((n, h, w, sc2), 63), "wt": ops.repack_conv_weight(r16((cout, c, 3, 3), 64, s)),
              "wsk": r16((cout, sc1 + sc2), 65, s), "b": r16((cout,), 66, 0.5), "bsk": r16((cout,), 67, 0.5)}

    def call(I, O, ws):
        return ok(L, L.ld_op_conv_skip(ptr(I["x"]), c, n, h, w, ptr(I["wt"]), ptr(I["b"]), ptr(I["s1"]), sc1, ptr(I["s2"]), sc2, ptr(I["wsk"]), ptr(I["bsk"]), None,
                                       ptr(O["y"]), cout, ptr(ws), ws.numel(), stream()), "ld_op_conv_skip")
    hold(ops, call, inputs, {"y": ((n, h, w, cout), H16)}, L.ld_op_conv_skip_ws_bytes(c, sc1, sc2, cout), route, f"conv_skip n{n} {h}x{w}")


# ------------------------------------------------------------------ norms

# (n, hw, c1, c2): shapes of tests/test_norm_gpu.py ragged against gn_num_chunks — HW < 8 (one chunk of 7 pixels), HW = 77 / 81 / 35 not
# divisible by their chunk counts, two sources
GN_SHAPES = [(1, 7, 64, 0), (3, 77, 96, 0), (1, 81, 320, 0), (2, 35, 320, 640)]


def _gn_inputs(n, hw, c1, c2):
    return {"x": r16((n, hw, c1), 81, 1.0, 0.3), "x2": r16((n, hw, c2), 82, 2.0, -0.5) if c2 else None, "gamma": r16((c1 + c2,), 83, 0.2, 1.0),
            "beta": r16((c1 + c2,), 84, 0.2)}


@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("n,hw,c1,c2", GN_SHAPES)
def test_groupnorm_footprint(L, ops, n, hw, c1, c2, silu):
    def call(I, O, ws):
        ok(L, L.ld_op_groupnorm(ptr(I["x"]), c1, ptr(I.get("x2")), c2, n, hw, ptr(I["gamma"]), ptr(I["beta"]), 1e-5, int(silu), ptr(O["y"]), ptr(ws), stream()),
           "ld_op_groupnorm")
        return L.ld_op_last_launches().decode()
    hold(ops, call, _gn_inputs(n, hw, c1, c2), {"y": ((n, hw, c1 + c2), H16)}, L.ld_op_groupnorm_ws_bytes(n, hw), lambda r: "gn_" in r, f"groupnorm {n}x{hw}x{c1}+{c2}")


@pytest.mark.parametrize("n,hw,c1,c2", GN_SHAPES)
def test_groupnorm_stats_footprint(L, ops, n, hw, c1, c2):
    chunks = L.ld_op_groupnorm_chunks(n, hw)
    inputs = {k: v for k, v in _gn_inputs(n, hw, c1, c2).items() if k in ("x", "x2")}

    def call(I, O, ws):
        ok(L, L.ld_op_groupnorm_stats(ptr(I["x"]), c1, ptr(I.get("x2")), c2, n, hw, ptr(O["part"]), stream()), "ld_op_groupnorm_stats")
        return L.ld_op_last_launches().decode()
    hold(ops, call, inputs, {"part": ((n * chunks * 64,), F32, dict(rows_behind=0))}, 0, None, f"groupnorm_stats {n}x{hw}x{c1}+{c2}")


@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("n,hw,c1,c2", GN_SHAPES)
def test_groupnorm_from_partials_footprint(L, ops, n, hw, c1, c2, silu):
    """The apply pass alone: the producer's partials are an fp32 input behind NaN / Inf guards."""
    gi = _gn_inputs(n, hw, c1, c2)
    part = ops.group_norm_stats(gi["x"], gi["x2"])
    pstat = part.shape[1]
    inputs = dict(gi, part=(part.reshape(-1), dict(rows_behind=0)))

    def call(I, O, ws):
        ok(L, L.ld_op_groupnorm_from_partials(ptr(I["x"]), c1, ptr(I.get("x2")), c2, n, hw, ptr(I["gamma"]), ptr(I["beta"]), 1e-5, int(silu), ptr(O["y"]),
                                              ptr(I["part"]), pstat, stream()), "ld_op_groupnorm_from_partials")
        return L.ld_op_last_launches().decode()
    hold(ops, call, inputs, {"y": ((n, hw, c1 + c2), H16)}, 0, None, f"groupnorm_from_partials {n}x{hw}x{c1}+{c2}")


@pytest.mark.parametrize("n,hw,c1,c2", GN_SHAPES)
def test_groupnorm_scale_shift_footprint(L, ops, n, hw, c1, c2):
    def call(I, O, ws):
        ok(L, L.ld_op_groupnorm_scale_shift(ptr(I["x"]), c1, ptr(I.get("x2")), c2, n, hw, ptr(I["gamma"]), ptr(I["beta"]), 1e-5, ptr(ws), 0, ptr(O["scale"]),
                                            ptr(O["shift"]), stream()), "ld_op_groupnorm_scale_shift")
        return L.ld_op_last_launches().decode()
    hold(ops, call, _gn_inputs(n, hw, c1, c2), {"scale": ((n, c1 + c2), F32), "shift": ((n, c1 + c2), F32)}, L.ld_op_groupnorm_ws_bytes(n, hw), None,
         f"groupnorm_scale_shift {n}x{hw}x{c1}+{c2}")


@pytest.mark.parametrize("rows,c", [(1, 8), (5, 520), (130, 320), (130, 2048)])      # tests/test_norm_gpu.py: one row; lane 0 alone with a second chunk; a last block half empty
def test_layernorm_footprint(L, ops, rows, c):
    inputs = {"x": r16((rows, c), 91, 2.0, 0.5), "gamma": r16((c,), 92, 0.2, 1.0), "beta": r16((c,), 93, 0.2)}

    def call(I, O, ws):
        ok(L, L.ld_op_layernorm(ptr(I["x"]), ptr(I["gamma"]), ptr(I["beta"]), ptr(O["y"]), rows, c, 1e-5, stream()), "ld_op_layernorm")
        return L.ld_op_last_launches().decode()
    hold(ops, call, inputs, {"y": ((rows, c), H16)}, 0, None, f"layernorm {rows}x{c}")


def test_harness_sees_a_row_too_many_on_the_device(L):
    """The harness against a real kernel's stores: ld_op_layernorm asked for rows + 1 rows on operands placed for `rows`.  The extra row is read
    from x's back guard (NaN) and stored into y's: reported as (y, back, row `rows`, column 0), every asked-for row written and right.  Both
    rows lie inside the test's own guarded buffers."""
    rows, c = 5, 320
    x, gamma, beta = r16((rows, c), 91, 2.0, 0.5), r16((c,), 92, 0.2, 1.0), r16((c,), 93, 0.2)
    want = torch.empty(rows, c, dtype=H16, device=DEV)
    ok(L, L.ld_op_layernorm(ptr(x), ptr(gamma), ptr(beta), ptr(want), rows, c, 1e-5, stream()), "ld_op_layernorm")
    px, py = FP.place(x, "nan", name="x"), FP.place_output((rows, c), H16, DEV)
    ok(L, L.ld_op_layernorm(ptr(px.view), ptr(gamma), ptr(beta), ptr(py.view), rows + 1, c, 1e-5, stream()), "ld_op_layernorm")
    torch.cuda.synchronize()
    assert FP.check_guards(py) == FP.Touch("y", "back", 0, rows, 0)
    assert FP.check_written(py) is None and FP.first_difference(py, want) is None and FP.check_guards(px) is None


# ------------------------------------------------------------------ executor workspace history

def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.uint8)


def _same(a, b, what):
    torch.cuda.synchronize()
    for i, (x, y) in enumerate(zip(a, b)):
        assert bool(torch.isfinite(x.float()).all()), f"{what}: output {i} of the small shape is not finite"
        assert torch.equal(_bits(x), _bits(y)), f"{what}: output {i} differs, first at flat index {int((_bits(x) != _bits(y)).flatten().nonzero()[0])}"


def _history(what, handles, large, small):
    """large(handle), small(handle) -> outputs.  Handle 1: large, small, small; handle 2: small.  All small results are the same bits."""
    h1, h2 = handles
    large(h1)
    first = small(h1)
    alone = small(h2)
    _same(first, alone, f"{what}: the small shape behind the large one against a handle that never saw the large one")
    _same(small(h1), alone, f"{what}: the small shape a second time")


def _rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


def test_unet_workspace_history(L, make):
    """Batch 4 at 16x16 with 154 context tokens on adverse inputs, then batch 1 at 7x9 with 77 tokens (63 self-attention keys, context rows
    77 .. Tp, ragged GroupNorm chunks, the counters of the row-resident convolution) and the CFG pair on it."""
    from lightdiffusion_amd._lib import F32 as LD_F32, FWD_PAIR, OK
    fam = FAMILIES["unet"]
    handles = [make(fam, loaded=True) for _ in range(2)]
    for hd in handles:
        assert L.ld_unet_reserve(hd, 4, 16, 16, 154) == OK
    xl, cl, sl = A.big((4, 4, 16, 16), 1).float(), A.outlier((4, 154, 64), 2).float() * 16.0, torch.full((4,), 10.0, device=DEV)
    xs, ss, c1, c2 = _rand((1, 4, 7, 9), 3), torch.ones(1, device=DEV), _rand((1, 77, 64), 4), _rand((2, 77, 64), 5)

    def large(hd):
        out = torch.empty(4, 4, 16, 16, device=DEV)
        assert L.ld_unet_set_context(hd, cl.data_ptr(), LD_F32, 4, 154, stream()) == OK
        assert L.ld_unet_forward(hd, xl.data_ptr(), sl.data_ptr(), out.data_ptr(), 4, 16, 16, 0, None, stream()) == OK

    def small(hd):
        o1, o2 = torch.full((1, 4, 7, 9), float("nan"), device=DEV), torch.full((2, 4, 7, 9), float("nan"), device=DEV)
        assert L.ld_unet_set_context(hd, c1.data_ptr(), LD_F32, 1, 77, stream()) == OK
        assert L.ld_unet_forward(hd, xs.data_ptr(), ss.data_ptr(), o1.data_ptr(), 1, 7, 9, 0, None, stream()) == OK
        assert L.ld_unet_set_context(hd, c2.data_ptr(), LD_F32, 2, 77, stream()) == OK
        assert L.ld_unet_forward(hd, xs.data_ptr(), ss.data_ptr(), o2.data_ptr(), 1, 7, 9, FWD_PAIR, None, stream()) == OK
        return o1, o2
    _history("unet", handles, large, small)


def test_controlnet_workspace_history():
    """The control branch: batch 4 at 16x16 with 154 context tokens and a hint batch of 2 on adverse inputs, then batch 1 at 7x9 with 77 tokens
    and its own hint, and the CFG pair on it — the residual buffers, the encoded hint and the arena the hint encoder shares all hold the large
    call's rows by then.  The small calls' hint and 13 residuals are the bits of a handle that never saw the large one.  (Every call stays
    inside the reserved plan: nothing re-reserves, and the hint is set anew for each latent size, as the branch demands.)"""
    from lightdiffusion_amd import weights as W
    from lightdiffusion_amd.controlnet import synthetic_controlnet
    cfg = W.tiny_unet_config()
    handles = [synthetic_controlnet(cfg, max_batch=4, max_hw=(16, 16), max_tokens=154) for _ in range(2)]
    epochs = [hd.reserve_epoch for hd in handles]
    xl, cl, sl = A.big((4, 4, 16, 16), 1).float(), A.outlier((4, 154, 64), 2).float() * 16.0, torch.full((4,), 10.0, device=DEV)
    hl = torch.ones(2, 3, 128, 128, device=DEV)
    xs, ss, c1, c2 = _rand((1, 4, 7, 9), 3), torch.ones(1, device=DEV), _rand((1, 77, 64), 4), _rand((2, 77, 64), 5)
    hs = torch.rand(1, 3, 56, 72, generator=torch.Generator().manual_seed(6)).to(DEV)

    def large(hd):
        hd.set_context(cl)
        hd.set_hint(hl)
        hd.forward(xl, sl)

    def small(hd):
        hd.set_context(c1)
        hd.set_hint(hs)
        enc = hd.hint()
        hd.forward(xs, ss)
        r1 = hd.residuals()
        hd.set_context(c2)
        hd.forward_pair(xs, ss)
        r2 = hd.residuals()
        assert all(r.shape[0] == 1 for r in r1) and all(r.shape[0] == 2 for r in r2) and len(r1) == len(r2) == hd.residual_count + 1
        return [enc] + r1 + r2
    _history("controlnet", handles, large, small)
    assert [hd.reserve_epoch for hd in handles] == epochs, "a call inside the reserved plan moved the workspace"


def _sized_history(L, make, name, entry, big_shape, small_shape, ins, outs):
    """A family whose run is entry(handle, inputs..., outputs..., b, h, w, stream): ins / outs(b, h, w, adverse) -> tensors."""
    from lightdiffusion_amd._lib import OK
    fam = FAMILIES[name]
    handles = [make(fam, loaded=True, reserved=big_shape) for _ in range(2)]
    fn = getattr(L, f"ld_{name}_{entry}")

    def run(hd, shape, adverse):
        i, o = ins(*shape, adverse), outs(*shape)
        assert fn(hd, *(ptr(t) for t in i), *(ptr(t) for t in o), *shape, stream()) == OK
        return o
    _history(f"{name} {entry}", handles, lambda hd: run(hd, big_shape, True), lambda hd: run(hd, small_shape, False))


def _nan(shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), device=DEV) if dtype == torch.float32 else torch.full(shape, 0xAA, dtype=dtype, device=DEV)


def test_vae_decode_workspace_history(L, make):
    """2 x 16x16 latents on adverse inputs, then 1 x 5x7: 35 attention keys in the masked last key tile, ragged GroupNorm chunks and conv tiles."""
    _sized_history(L, make, "vae", "decode", (2, 16, 16), (1, 5, 7), lambda b, h, w, adv: [A.big((b, 4, h, w), 6).float() if adv else _rand((b, 4, h, w), 7)],
                   lambda b, h, w: [_nan((b, 8 * h, 8 * w, 3))])


def test_vae_encode_workspace_history(L, make):
    _sized_history(L, make, "vae", "encode", (2, 16, 16), (1, 3, 5),
                   lambda b, h, w, adv: [A.big((b, 3, 8 * h, 8 * w), 8).float() if adv else torch.rand(b, 3, 8 * h, 8 * w, generator=torch.Generator().manual_seed(9)).to(DEV) * 2 - 1],
                   lambda b, h, w: [_nan((b, 8, h, w))])


def test_esrgan_workspace_history(L, make):
    """2 x 32x32 on adverse inputs, then 1 x 5x7: under one tile, the dense buffers' pitch gaps and the up-convolutions' arena hold the large run."""
    _sized_history(L, make, "esrgan", "forward", (2, 32, 32), (1, 5, 7),
                   lambda b, h, w, adv: [A.big((b, h, w, 3), 10).float() if adv else torch.rand(b, h, w, 3, generator=torch.Generator().manual_seed(11)).to(DEV)],
                   lambda b, h, w: [_nan((b, 4 * h, 4 * w, 3))])


def test_taesd_workspace_history(L, make):
    _sized_history(L, make, "taesd", "decode", (2, 16, 16), (1, 5, 7), lambda b, h, w, adv: [A.big((b, h, w, 4), 12).float() if adv else _rand((b, h, w, 4), 13)],
                   lambda b, h, w: [_nan((b, 8 * h, 8 * w, 3)), _nan((b, 8 * h, 8 * w, 3), torch.uint8)])


def test_clip_scratch_history(ops):
    """The text model has no handle: its operator calls share the wrappers' scratch.  One prompt, then three prompts on the adverse weights (the
    split-K slabs and every intermediate hold large magnitudes), then the one prompt twice more: the same bits each time."""
    import clip_chain as CC
    from lightdiffusion_amd.clip import CLIPTextModelHIP
    cfg = CC.config("tiny")
    tm = CLIPTextModelHIP(cfg, CC.state_dict(cfg), device=DEV)
    hot = CLIPTextModelHIP(cfg, CC.state_dict(cfg, A.source("clip", gain=A.CHAIN_GAIN[("clip", "tiny")])), device=DEV)
    one, three = CC.prompts(1, seed=1), CC.prompts(3, seed=2)
    alone = tm(one, intermediate_output=-2)
    hot(three, intermediate_output=-2)
    _same(tm(one, intermediate_output=-2), alone, "clip: one prompt behind three adverse ones")
    _same(tm(one, intermediate_output=-2), alone, "clip: one prompt a second time")
