"""Element-wise error bounds and a signed-bias statistic for the HIP kernels' outputs (helper module of the route tests).

Why not rel-L2 alone: fp16 storage costs ~3e-4 of rel-L2, so a 2e-3 budget hides a wrong tile corner, a halo pixel, a missing bias in one
column, an error confined to the last ragged tile, and any systematic bias below ~1e-3.  Here every element is held to a bound derived from
the kernel's rounding points, against a reference computed in fp64 from the same fp16 inputs, and the mean signed error is held to 2^-11 / 8.

Rounding model (fp16 inputs, fp32 MFMA accumulation, one fp16 rounding of the output, round to nearest):
  * fp16 x fp16 products are exact in fp32; the matrix core accumulates them as an fp32 chain.  Its error against fp64 is c_acc(K) * sum|a b|
    (c_acc below), where sum|a b| = (|A| |W|^T) of the same row / column.
  * the GEMM epilogues stage the finished tile (alpha acc + bias) in fp16, apply the activation to the fp16 values, and add rowvec /
    residual as packed fp16 adds (gemm_device.h epilogue_tile, add8h): one fp16 rounding of alpha acc and of the pre-activation value (2^-11 each,
    times the activation's Lipschitz constant L_act <= 1.13 for SiLU / quick-GELU / GELU), one of the activation's output before a residual,
    one per packed add (rowvec, then residual), fp32 arithmetic in between (2^-23), plus the approximation error eps_act of an activation fit.
  * the output is rounded to fp16 once more: 2^-11 |y_hat| (normal range) or 2^-25 absolute (subnormal range): the 2^-11 |y_hat| + 2^-24 terms.
  * every extra fp16 rounding on the way (a normalised or folded operand, the attention's scaled Q and its P tile) adds 2^-11 of that
    intermediate, propagated to the output; the callers below state theirs.
"""
from __future__ import annotations

import math

import torch

U = 2.0 ** -11            # fp16 unit roundoff (half an ulp, relative)
TINY = 2.0 ** -24         # absolute floor: fp16 subnormal rounding (2^-25) with room
BIAS_TOL = U / 8          # |mean signed error| / mean |y_hat| allowed (RTN: ~1e-6 at >= 1e4 elements; RTZ: ~-3e-4)
L_ACT = 1.13              # max |d act / dx| of SiLU (1.10), quick-GELU (1.10), erf-GELU (1.13)
GELU_FIT_ABS = 5.1e-7     # common.h: max |error| of the kernels' GELU fit (absolute)
GELU_FIT_BIAS = 5e-5      # common.h: relative error of the fit where |gelu| > 1e-3 (the fit's own bias allowance)


def c_acc(K: int) -> float:
    """Accumulation error of a K-long fp32 MFMA chain per unit of sum|a b|.  The fp64 comparison of the f32 fma chain on this chip measures
    0.75-1.5e-7 at K <= 1024 and 3.5e-7 at K = 4096 (a random walk: it grows as sqrt(K)); the model 1.5e-7 * max(1, sqrt(K / 1024)) with the
    permitted factor 2 on top.  A split over K adds one fp32 sum per slice of already-rounded partials: inside the same factor."""
    return 2.0 * 1.5e-7 * max(1.0, math.sqrt(K / 1024.0))


def bias_kept_fraction(ref: torch.Tensor, floor_frac: float = 1e-3) -> float:
    """Share of the elements the bias statistic keeps (|y_hat| above floor_frac * max|y_hat|)."""
    a = ref.double().abs()
    return float((a > floor_frac * float(a.max())).double().mean())


def rtn_noise(n: float) -> float:
    """What the bias statistic of n elements may show by chance under round to nearest: four standard deviations of the mean of n independent
    relative rounding errors, each uniform within +-U (standard deviation U / sqrt(3)).  1.1e-5 at 1e4 elements — inside BIAS_TOL's own room —
    but 1e-4 at a 100-element output, which the fixed tolerance alone would fail one time in ten."""
    return 4.0 * U / math.sqrt(3.0 * max(1.0, n))


def rtn_noise_weighted(mags: torch.Tensor, ref: torch.Tensor, floor_frac: float = 1e-3) -> float:
    """rtn_noise for an output whose roundings are NOT relative to |y_hat|: element i carries independent round-to-nearest errors of values of
    magnitude mags_i in total (each uniform within +-U of its value: standard deviation at most U mags_i / sqrt(3)), so the bias statistic
    sum(e_i sign_i) / sum|y_hat_i| over the kept elements has standard deviation U / sqrt(3) * sqrt(sum mags_i^2) / sum|y_hat_i|; four of
    them.  With mags = |y_hat| this is rtn_noise(n_eff) of independent_roundings' n_eff.  It is what a residual that cancels the contraction
    needs (tests/adverse.py cancel: the packed adds round relative to |pre| = 8 |y_hat|) and what heavy-tailed outputs need (few elements carry
    the sum)."""
    a = ref.double().abs().flatten()
    m = mags.double().abs().flatten().to(a.device)
    k = a > floor_frac * float(a.max())
    if int(k.sum()) == 0:
        return 0.0
    return float(4.0 * U / math.sqrt(3.0) * (m[k] * m[k]).sum().sqrt() / a[k].sum())


def independent_roundings(ref: torch.Tensor, keep: torch.Tensor | None = None, floor_frac: float = 1e-3) -> float:
    """The n of rtn_noise for an output.  The bias statistic is the |y_hat|-weighted mean of the kept elements' relative rounding errors, and equal
    values round equally, so its chance level is that of  n_eff = (sum W_v)^2 / sum W_v^2  independent errors, W_v the summed |y_hat| of each
    DISTINCT kept value v: the element count for distinct values of one size, 1 for a softmax whose rows are all three tied maxima (p = 1/3, each
    rounded down by 2.4e-4), about five for rows of m = 1 .. 6 tied maxima however many rows there are."""
    a = ref.double().abs().flatten()
    k = (a > floor_frac * float(a.max())) if keep is None else (keep.flatten().to(a.device) & (a > 0))
    if int(k.sum()) == 0:
        return 1.0
    vals, inv = torch.unique(a[k], return_inverse=True)
    w = torch.zeros_like(vals).scatter_add_(0, inv, a[k])
    return float(w.sum() ** 2 / (w * w).sum())


def subnormal_bias_allowance(ref: torch.Tensor, keep: torch.Tensor) -> float:
    """What fp16's subnormal range may add to the bias statistic over `keep`: below 2^-14 the rounding error is absolute, up to 2^-25 per element,
    and does not average out against |y_hat| (everything below 2^-25 rounds DOWN to zero) — mean(2^-25 over the kept subnormal elements) /
    mean |y_hat|.  Zero for an output in the normal range; it voids the statistic where most kept values are subnormal (a 4096-column softmax
    of scale-4 scores: the median probability is 8e-8), where the element bound alone holds the kernel."""
    a = ref.double().abs().flatten()
    k = keep.flatten().to(a.device) & (a > 0)
    if int(k.sum()) == 0:
        return 0.0
    return float(((a[k] < 2.0 ** -14).double() * 2.0 ** -25).mean() / a[k].mean())


def top_half_per_row(ref: torch.Tensor) -> torch.Tensor:
    """Mask of the largest 50 % of every row of `ref` (the softmax's bias statistic: a row's small probabilities are fp16 subnormals)."""
    k = max(1, ref.shape[-1] // 2)
    thr = ref.double().topk(k, dim=-1).values[..., -1:]
    return ref.double() >= thr


def signed_bias(y: torch.Tensor, ref: torch.Tensor, floor_frac: float = 1e-3, keep: torch.Tensor | None = None) -> float:
    """s = mean((y - y_hat) sign(y_hat)) / mean(|y_hat|) over the elements with |y_hat| above floor_frac * max|y_hat| (and inside `keep`)."""
    y, ref = y.double().flatten(), ref.double().flatten().to(y.device)
    a = ref.abs()
    if keep is not None:
        keep = keep.flatten().to(y.device) & (a > 0)
    else:
        keep = a > floor_frac * float(a.max())
    if int(keep.sum()) == 0:
        return 0.0
    return float(((y - ref)[keep] * ref[keep].sign()).mean() / a[keep].mean())


def locate(index: int, shape, image_rows: int | None = None, width: int | None = None, tile=None) -> str:
    """'(image i, row r, column c), tile (tm, tn)' of flat element `index` of a [M][N] result whose rows are images of image_rows pixels
    (a row of `width` pixels each); other shapes: the plain multi-index."""
    idx = []
    rem = index
    for s in reversed(shape):
        idx.append(rem % s)
        rem //= s
    idx = idx[::-1]
    if len(shape) != 2:
        return "element " + str(tuple(int(i) for i in idx))
    m, n = int(idx[0]), int(idx[1])
    if image_rows:
        img, pix = divmod(m, image_rows)
        where = f"(image {img}, row {pix // width if width else pix}, column {pix % width if width else 0}; channel {n})"
    else:
        where = f"(row {m}, column {n})"
    if tile is not None:
        where += f", tile ({m // tile[0]}, {n // tile[1]}) of {tile[0]}x{tile[1]}"
    return where


def check(y: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor, what: str, *, image_rows=None, width=None, tile=None,
          bias_extra: float = 0.0, floor_frac: float = 1e-3, keep: torch.Tensor | None = None):
    """Assert |y - y_hat| <= bound element-wise and |signed_bias| <= BIAS_TOL + bias_extra.  Both criteria are evaluated and reported
    together; the message names the worst element, its tile and the ratio error / bound."""
    y = y.to(ref.device).double()
    ref = ref.double()
    bound = torch.broadcast_to(bound.to(ref.device).double(), ref.shape)
    assert y.shape == ref.shape, (y.shape, ref.shape)
    fails = []
    if not bool(torch.isfinite(y).all()):
        fails.append(f"{int((~torch.isfinite(y)).sum())} non-finite outputs")
    err = (y - ref).abs()
    ratio = torch.nan_to_num(err / bound, nan=float("inf"))
    worst = int(ratio.flatten().argmax())
    r = float(ratio.flatten()[worst])
    if r > 1.0:
        nbad = int((ratio > 1.0).sum())
        fails.append(f"element bound: {nbad} of {ratio.numel()} outside, worst {locate(worst, tuple(ref.shape), image_rows, width, tile)}: "
                     f"got {float(y.flatten()[worst]):.6g}, fp64 {float(ref.flatten()[worst]):.6g}, error / bound = {r:.3g}")
    s = signed_bias(y, ref, floor_frac, keep)
    tol = BIAS_TOL + bias_extra
    if abs(s) > tol:
        fails.append(f"signed bias {s:.3g} outside +-{tol:.3g} (a systematic rounding or scaling error)")
    assert not fails, f"{what}: " + "; ".join(fails)
    return r, s


# ------------------------------------------------------------------ references and bounds of the contraction families

def _act(t: torch.Tensor, act: str) -> torch.Tensor:
    if act == "silu":
        return t * torch.sigmoid(t)
    if act == "quick_gelu":
        return t * torch.sigmoid(1.702 * t)
    if act == "gelu":
        return 0.5 * t * (1.0 + torch.erf(t / math.sqrt(2.0)))
    return t


def epilogue_ref(acc, absdot, K, bias=None, residual=None, alpha=1.0, act="none", extra=None, rowvec=None, staged_subnormal=True):
    """y_hat and its element bound for y = act(alpha * acc + bias) + residual (act 'geglu': acc / absdot hold [value | gate] halves).
    acc, absdot: fp64 A W^T and |A| |W|^T; `extra`: an fp64 tensor of further input-side error of acc (e.g. a rounded normalised operand).
    The staged fp16 tile rounds to 2^-11 |pre| in fp16's normal range and to 2^-25 ABSOLUTE below 2^-14, where 2^-11 |pre| is less than that:
    the tile's term is max(2^-11 |pre|, 2^-25) — unchanged for every |pre| >= 2^-14.  It matters where something multiplies the staged value
    afterwards: a GEGLU whose value half is subnormal times a gate of several hundred (tests/test_adverse_cpu.py holds that the bound is wrong
    without it and still rejects a tile flushed to zero with it).  staged_subnormal=False: the bound without that floor (that control only)."""
    e_acc = c_acc(K) * absdot * abs(alpha)
    if extra is not None:
        e_acc = e_acc + extra * abs(alpha)
    pre = alpha * acc + (0.0 if bias is None else bias.double())
    e_pre = e_acc + (U + 2.0 ** -23) * ((alpha * acc).abs() + pre.abs())      # the staged fp16 tile (and an fp16 bias add)
    if staged_subnormal:
        e_pre = e_pre + (2.0 ** -25 - U * pre.abs()).clamp_min(0.0)
    if act == "geglu":
        n2 = pre.shape[-1] // 2
        a, g = pre[..., :n2], pre[..., n2:]
        ea, eg = e_pre[..., :n2], e_pre[..., n2:]
        ga = _act(g, "gelu")
        y = a * ga
        b = ga.abs() * ea + (a.abs() + ea) * (L_ACT * eg + GELU_FIT_ABS) + (U + 2.0 ** -23) * y.abs()   # (+ gelu(g) rounded to fp16)
    else:
        y = _act(pre, act)
        b = (L_ACT if act != "none" else 1.0) * e_pre
    for add in (rowvec, residual):                                          # packed fp16 adds, each onto an fp16-rounded value
        if add is not None:
            b = b + U * y.abs()
            y = y + add.double()
    return y, U * y.abs() + b + TINY


def linear_ref(x, w, bias=None, residual=None, alpha=1.0, act="none"):
    """fp64 reference of ld_op_linear on the device: y_hat, bound.  GEGLU: w / bias rows [value | gate] as in the checkpoint."""
    xd, wd = x.double(), w.double()
    acc = xd @ wd.t()
    absdot = xd.abs() @ wd.abs().t()
    return epilogue_ref(acc, absdot, x.shape[-1], bias, residual, alpha, act)


DOWNSAMPLE_PAD = (0, 1, 0, 1)     # the VAE encoder's Downsample (LD.py:3514-3528): F.pad's (left, right, top, bottom), then a 3x3 stride-2 conv, no padding


def conv_out_hw(hv: int, wv: int, ksize: int, stride: int, pad=None):
    """(ho, wo) of a ksize x ksize convolution at `stride` over an hv x wv image padded by pad = (left, right, top, bottom), None = ksize // 2 all round."""
    l, r, t, b = (ksize // 2,) * 4 if pad is None else pad
    return (hv + t + b - ksize) // stride + 1, (wv + l + r - ksize) // stride + 1


def im2col(x_nhwc: torch.Tensor, ksize: int, stride: int = 1, out_hw=None, pad=None) -> torch.Tensor:
    """fp64 im2col of an NHWC fp16 tensor (after an optional nearest resize to out_hw): [n * ho * wo][C * k * k], columns (c, ky, kx) —
    the order of a [Cout][C][k][k] weight reshaped to [Cout][C k k].  pad: (left, right, top, bottom) zeros as F.pad takes them (None: k // 2)."""
    x = x_nhwc.permute(0, 3, 1, 2).double()
    if out_hw is not None and tuple(out_hw) != tuple(x.shape[-2:]):
        x = torch.nn.functional.interpolate(x, size=tuple(out_hw), mode="nearest")
    if pad is None:
        cols = torch.nn.functional.unfold(x, ksize, padding=ksize // 2, stride=stride)     # [n][C k k][L]
    else:
        cols = torch.nn.functional.unfold(torch.nn.functional.pad(x, tuple(pad)), ksize, padding=0, stride=stride)
    return cols.transpose(1, 2).reshape(-1, cols.shape[1])


def conv_ref(x, w_oihw, bias=None, residual=None, stride=1, out_hw=None, x2=None, rowvec=None, pad=None):
    """fp64 reference of ld_op_conv (NHWC, pad k // 2, or pad = (left, right, top, bottom)) as explicit im2col + matmul on the device:
    y_hat [n*ho*wo][Cout], bound, (ho, wo)."""
    xin = x if x2 is None else torch.cat([x, x2], dim=-1)
    k = w_oihw.shape[-1]
    cols = im2col(xin, k, stride, out_hw, pad)
    wm = w_oihw.double().reshape(w_oihw.shape[0], -1)
    acc = cols @ wm.t()
    absdot = cols.abs() @ wm.abs().t()
    hv, wv = (x.shape[1], x.shape[2]) if out_hw is None else out_hw
    ho, wo = conv_out_hw(hv, wv, k, stride, pad) if pad is not None else ((hv - 1) // stride + 1, (wv - 1) // stride + 1) if k == 3 else (hv, wv)
    rv = None if rowvec is None else rowvec.double().repeat_interleave(ho * wo, dim=0)
    res = None if residual is None else residual.reshape(-1, residual.shape[-1])
    y, bd = epilogue_ref(acc, absdot, wm.shape[1], bias, res, rowvec=rv)
    return y, bd, (ho, wo)


def boundary_rows(M: int, bm: int, per_image: int | None = None, width: int | None = None):
    """Row indices covering every tile-boundary class: first / last row of the first tiles and of the last full tile, the last ragged
    tile, and per image its first / last pixel, the ends of its first and last pixel rows (the image corners)."""
    rows = {0, 1, M - 1, M - 2}
    for t in (0, 1, M // bm - 1, M // bm):
        for o in (0, bm - 1):
            rows.add(t * bm + o)
    if per_image:
        for i in range(M // per_image):
            base = i * per_image
            rows.update({base, base + per_image - 1})
            if width:
                rows.update({base + width - 1, base + per_image - width})
    return sorted(r for r in rows if 0 <= r < M)


def cpu_rows_linear(x, w, rows):
    """CPU fp64 A W^T of the sampled rows (an independent evaluation of the device reference)."""
    return x[rows].cpu().double() @ w.cpu().double().t()


def cpu_rows_conv(x, w_oihw, rows, stride=1, out_hw=None, x2=None, pad=None):
    """CPU fp64 convolution at the sampled output pixels (rows of the [n*ho*wo] result), by explicit patch gathering.
    pad = (left, right, top, bottom): the zeros around the image (None: k // 2 all round)."""
    xin = (x if x2 is None else torch.cat([x, x2], dim=-1)).cpu()
    n, h, wd, c = xin.shape
    hv, wv = (h, wd) if out_hw is None else out_hw
    k = w_oihw.shape[-1]
    ho, wo = conv_out_hw(hv, wv, k, stride, pad) if pad is not None else ((hv - 1) // stride + 1, (wv - 1) // stride + 1) if k == 3 else (hv, wv)
    left, top = (k // 2, k // 2) if pad is None else (pad[0], pad[2])
    wm = w_oihw.cpu().double()
    out = []
    for r in rows:
        img, pix = divmod(r, ho * wo)
        oy, ox = divmod(pix, wo)
        acc = torch.zeros(wm.shape[0], dtype=torch.float64)
        for ky in range(k):
            for kx in range(k):
                vy, vx = oy * stride + ky - top, ox * stride + kx - left
                if 0 <= vy < hv and 0 <= vx < wv:
                    sy, sx = (vy * h) // hv, (vx * wd) // wv           # nearest resize: source pixel floor(v * in / out)
                    acc += wm[:, :, ky, kx] @ xin[img, sy, sx].double()
        out.append(acc)
    return torch.stack(out)


def linear_batched_ref(x, w, bias=None, bias_m=None, n_valid=None, alpha=1.0):
    """fp64 reference of ld_op_linear_batched: x [b][M][K], w [b][N][K] (or [N][K], shared), bias [N], bias_m [M] (along the rows of y),
    only the first n_valid rows of w exist -> y_hat [b][M][n_valid], bound (epilogue_ref's, bias_m as a second bias of the staged tile).
    The stored columns n_valid .. N-1 are NOT part of the reference; what they hold is fixed by the kernels (gemm3.hip gemm3_kernel /
    gemm4_kernel loaders: `n = n0 + row < p.n_valid ? n0 + row : p.n_valid - 1`; the epilogue stores every n < N): the loader reads row
    n_valid - 1 in place of a row that does not exist, so each pad column repeats column n_valid - 1 — a finite value, bit for bit that column
    when there is no per-column bias (pad_columns_held).  They are never zeros of their own, and nothing behind may count on that: the softmax
    over `valid` keys overwrites the scores' pad columns with exact zeros, and P V then runs over all Lp columns of P against a finite V^T."""
    xd, wd = x.double(), w.double()
    nv = wd.shape[-2] if n_valid is None else n_valid
    wd = wd[..., :nv, :]
    acc = xd @ wd.transpose(-1, -2)
    absdot = xd.abs() @ wd.abs().transpose(-1, -2)
    b = None
    if bias is not None:
        b = bias.double()[:nv]
    if bias_m is not None:
        b = (0.0 if b is None else b) + bias_m.double().reshape(-1, 1)
    return epilogue_ref(acc, absdot, x.shape[-1], b, None, alpha)


def pad_columns_held(y, n_valid, what):
    """The stored pad columns of a batched linear without a per-column bias: each a bitwise repeat of column n_valid - 1 (linear_batched_ref)."""
    if y.shape[-1] > n_valid:
        last = y[..., n_valid - 1:n_valid]
        assert bool(torch.isfinite(y[..., n_valid:].float()).all()) and torch.equal(y[..., n_valid:], last.expand_as(y[..., n_valid:])), \
            f"{what}: the {y.shape[-1] - n_valid} pad columns do not repeat column {n_valid - 1}"


def pv_ref(p, vt, valid):
    """fp64 O = P V for P [b][L][Lp] (softmax rows whose columns valid .. Lp-1 MUST be exactly zero: asserted) and V^T [b][C][Lp], over the
    valid keys only — the pad columns of V^T may hold anything finite: y_hat [b][L][C], bound."""
    assert bool((p[..., valid:] == 0).all()), "P's pad columns are not exactly zero"
    assert bool(torch.isfinite(vt.float()).all()), "V^T holds a non-finite value (0 * inf in the pad columns)"
    return linear_batched_ref(p[..., :valid], vt[..., :valid])


def attention_ref(q, k, v, heads, causal=False, ones=None, p_subnormal=False):
    """fp64 softmax(q k^T / sqrt(d)) v on the device from the fp16 inputs ([b][L][heads d]) and its element bound:
        2 * 2^-11 |o_hat|                      output rounding + P's rounding against an unrounded denominator (what the kernels without the ones
                                              column did until their denominator summed the rounded weights as well: room now, kept as it was)
      + 2^-11 sum p |v - o_hat| / sum p          P rounded to fp16 (RTN: relative 2^-11 per weight)
      + sum p |ds| |v - o_hat| / sum p           Q * scale * log2(e) rounded once: |ds_j| <= 2^-11 scale sum_c |q_c| |k_jc|
      + c_acc(Lk) sum p |v| / sum p + 2^-24     fp32 accumulation of O and the fp32 reciprocal
      + 2^-25 sum_{j in S} (|v_j| + |o_hat|)     P's subnormal range, S = {j: (s_j - max s) log2(e) < -14}: the kernels round P_j = 2^(s_j - m_ref)
                                              to fp16 relative to a reference m_ref <= max s, so a weight computed below 2^-14 — only keys of
                                              S can be — carries an ABSOLUTE error of up to 2^-25 (everything below 2^-25 becomes 0), not a
                                              relative 2^-11; later moves of the reference only shrink it, and the denominator is >= 1 (the
                                              maximum's own weight).  |v_j| + |o_hat| covers either denominator (the rounded P, as the
                                              ones column and l_run sum it, or the unrounded).  Only with p_subnormal=True (the peaked tests): on scores at
                                              scale 1 S is empty but for one or two keys of a few d <= 16 rows (a spread of 15.6 exp2 units
                                              at most over ATTN_ROUTES), and those rows keep the bound they had; under peaked scores S is
                                              most keys of a row: 250 keys each 2^-20 of the peak move a |o_hat| of 2e-6 by 4e-7.
    Observed on the MI355X over ATTN_PEAKED (tests/test_routes_gpu.py), worst error / bound and largest signed bias per pattern family, with
    the same figures of the fp32 emulation of the recursion (tests/test_errbound_cpu.py) behind them:
        spike    0.269,  2.0e-5   (emulation 0.255,  1.8e-5)        stairs   0.326, -2.5e-5   (emulation 0.326,  8.9e-6)
        descend  0.318, -2.3e-5   (emulation 0.318, -2.0e-5)        onehot   0.405,  3.6e-5   (emulation 0.405, -2.8e-5)
        offset   0.080, -2.5e-5   (emulation 0.059,  1.4e-5; with q0 = 4 sqrt(d) itself, whose scaled value rounds 2.2e-4 low in every row alike,
                                   the bias was -2.35e-4 / -1.55e-4: attn_patterns._offset_q0 picks a q0 whose scaled value is an fp16 number)
    all inside the plain BIAS_TOL.
    Without the subnormal term one element of 262144 of flash_attn512_kernel<512,plain> under spike stood at error / bound 1.002, and the
    emulation returned the same fp16 number.  (|v_j| + |o_hat| rather than |v_j - o_hat|: against the unrounded denominator l_run the error is
    sum err_j v_j, which |v_j - o_hat| does not cover where the v_j are alike; and no [Lq][Lk][d] temporary, as above.)"""
    b, lq, c = q.shape
    lk = k.shape[1]
    d = c // heads
    qd = q.double().reshape(b, lq, heads, d).transpose(1, 2)
    kd = k.double().reshape(b, lk, heads, d).transpose(1, 2)
    vd = v.double().reshape(b, lk, heads, d).transpose(1, 2)
    scale = 1.0 / math.sqrt(d)
    s = (qd @ kd.transpose(-1, -2)) * scale
    ds = U * scale * (qd.abs() @ kd.abs().transpose(-1, -2)) + 2.0 ** -22 * s.abs()
    if causal:
        mask = torch.ones(lq, lk, dtype=torch.bool, device=q.device).triu(1)
        s = s.masked_fill(mask, float("-inf"))
        ds = ds.masked_fill(mask, 0.0)
    p = torch.softmax(s, dim=-1)
    o = p @ vd
    pv = p @ vd.abs()
    # (sum p |v - o_hat| is taken as sum p |v| + |o_hat| sum p: no [Lq][Lk][d] temporary)
    t_p = U * (pv + o.abs())
    t_s = (p * ds) @ vd.abs() + (p * ds).sum(-1, keepdim=True) * o.abs()
    t_a = c_acc(lk) * pv
    bound = 2 * U * o.abs() + t_p + t_s + t_a + TINY
    if p_subnormal:
        sub = (((s - s.amax(-1, keepdim=True)) * 1.4426950408889634 < -14.0) & torch.isfinite(s)).double()
        bound = bound + 2.0 ** -25 * (sub @ vd.abs() + sub.sum(-1, keepdim=True) * o.abs())
    back = lambda t: t.transpose(1, 2).reshape(b, lq, c)
    return back(o), back(bound)


# ------------------------------------------------------------------ references and bounds of the norm, boundary-conv and fold kernels
# (norm.hip, misc.hip).  Observed worst error / bound and signed bias per family on the MI355X: see each docstring's last line.

def _gn_stats(x1, x2, eps):
    """fp64 group statistics of the channel concat [n][HW][C] and their fp32 error model (see groupnorm_ref)."""
    x = (x1 if x2 is None else torch.cat([x1, x2], dim=-1)).double()
    n, c = x.shape[0], x.shape[-1]
    x = x.reshape(n, -1, c)
    cpg = c // 32
    xg = x.reshape(n, -1, 32, cpg)
    cnt = xg.shape[1] * cpg
    mu = xg.mean(dim=(1, 3))                                   # [n][32]
    msq = (xg * xg).mean(dim=(1, 3))
    e_mu = c_acc(cnt) * xg.abs().mean(dim=(1, 3))
    e_msq = c_acc(cnt) * msq
    var = (msq - mu * mu).clamp_min(0.0)
    e_cancel = 2.0 * mu.abs() * e_mu + 2.0 ** -23 * (msq + mu * mu)      # what var = msq - mu^2 adds to e_msq: grows as (mu / sigma)^2
    e_var = e_msq + e_cancel
    rstd = (var + eps).rsqrt()
    # d rstd / rstd for a var off by up to e_var (and clamped at 0): e_var / (2 (var + eps)) to first order; the downward side is taken
    # exactly, (1 - r)^-1/2 - 1 with r = min(e_var, var) / (var + eps) < 1, because a constant group has e_var >> var + eps
    r_dn = torch.minimum(e_var, var) / (var + eps)
    rel = torch.maximum((1.0 - r_dn).rsqrt() - 1.0, e_var / (2.0 * (var + eps))) + 2.0 ** -22
    rel_nocancel = torch.maximum((1.0 - torch.minimum(e_msq, var) / (var + eps)).rsqrt() - 1.0, e_msq / (2.0 * (var + eps))) + 2.0 ** -22
    per_c = lambda t: t.repeat_interleave(cpg, dim=1).unsqueeze(1)        # [n][32] -> [n][1][C]
    return x, per_c(mu), per_c(rstd), per_c(rel), per_c(e_mu), per_c(rel_nocancel)


def groupnorm_scale_shift_ref(x1, x2, gamma, beta, eps):
    """fp64 (sc, sh) [n][C] of y = x sc + sh, sc = rstd gamma, sh = beta - mu sc, with their bounds (no fp16 store: both are fp32):
        |d sc| <= |sc| (rel_rstd + 2^-23),   |d sh| <= |mu sc| (rel_rstd + 2^-22) + e_mu |sc| + 2^-23 |sh|     (rel_rstd, e_mu: groupnorm_ref).
    Observed on the MI355X: worst error / bound 0.32 (scale), 0.33 (shift), signed bias below 1e-6."""
    x, mu, rstd, rel, e_mu, _ = _gn_stats(x1, x2, eps)
    ga, be = gamma.double().to(x.device), beta.double().to(x.device)
    sc = rstd * ga
    sh = be - mu * sc
    b_sc = sc.abs() * (rel + 2.0 ** -23) + 1e-30
    b_sh = (mu * sc).abs() * (rel + 2.0 ** -22) + e_mu * sc.abs() + 2.0 ** -23 * sh.abs() + 1e-30
    return sc[:, 0], b_sc[:, 0], sh[:, 0], b_sh[:, 0]


def groupnorm_ref(x1, x2, gamma, beta, eps, silu, parts=False):
    """fp64 GroupNorm(32) (+SiLU) of the channel concat of NHWC x1, x2 ([n][..][C1], [n][..][C2]) from the fp16 inputs: y_hat [n][HW][C], bound.
    Rounding points of gn_stats_kernel / gn_apply_kernel (norm.hip):
      * fp32 sums of x and x^2 over cnt = HW C/32 values (per-thread chains, LDS and shuffle trees, a sweep over the chunk partials):
        e_mu = c_acc(cnt) mean|x|,  e_msq = c_acc(cnt) mean x^2;
      * var = msq - mu^2 in fp32:  e_var = e_msq + 2 |mu| e_mu + 2^-23 (msq + mu^2) — the cancellation term, growing as (mu / sigma)^2;
      * rstd = rsqrtf(var + eps):  rel_rstd = e_var / (2 (var + eps)) + 2^-22 (the downward side exactly, see _gn_stats);
      * y = x sc + sh with sc = rstd gamma, sh = beta - mu sc in fp32:
            |x - mu| rstd |gamma| rel_rstd + e_mu rstd |gamma| + 2^-23 (|x sc| + |mu sc| + |sh| + |y|)
        (|mu sc| beside |sh|: the product inside sh rounds relative to itself, and beta may cancel it in sh);
      * SiLU x / (1 + __expf(-x)): the linear bound times L_ACT, + 2^-21 |y| for exp / add / divide, + 2^-23 |x| |y| for the rounding of
        the exponential's argument (x log2 e) — only visible beyond |x| ~ 4;
      * the fp16 store: U |y| + TINY.
    parts=True: also returns the share of the bound that the cancellation term contributes, per element.
    Observed on the MI355X (tests/test_norm_gpu.py): worst error / bound 0.997 (the fp16 store; from re-chunked partials 0.985, mu / sigma = 30 and a
    constant group 0.986, the chunk partials of gn_stats_kernel alone 0.44), signed bias below 1e-5 from 2000 elements on, -6.7e-5 at a 64-element output."""
    x, mu, rstd, rel, e_mu, rel0 = _gn_stats(x1, x2, eps)
    ga, be = gamma.double().to(x.device), beta.double().to(x.device)
    sc = rstd * ga
    sh = be - mu * sc
    y = (x - mu) * sc + be
    fp32 = 2.0 ** -23 * ((x * sc).abs() + (mu * sc).abs() + sh.abs() + y.abs())
    lin = lambda r: (x - mu).abs() * sc.abs() * r + e_mu * sc.abs() + fp32
    b, b0 = lin(rel), lin(rel0)
    if silu:
        pre = y
        y = pre * torch.sigmoid(pre)
        act = (2.0 ** -21 + 2.0 ** -23 * pre.abs()) * y.abs()
        b, b0 = L_ACT * b + act, L_ACT * b0 + act
    store = U * y.abs() + TINY
    if parts:
        return y, b + store, (b - b0) / (b + store)
    return y, b + store


def layernorm_ref(x, gamma, beta, eps):
    """fp64 LayerNorm over the last dim from the fp16 inputs: y_hat, bound.  layernorm_kernel (norm.hip) holds the row in registers and takes
    two passes, mu then sum (x - mu)^2, so there is no cancellation term; what remains of a large mean is the fp32 sum's own error:
      * e_mu = c_acc(C) mean|x|; every d = x - mu carries it, and since sum d = 0 the variance sees it only as e_mu^2:
        rel_rstd = (c_acc(C) var + e_mu^2) / (2 (var + eps)) + 2^-22;
      * y = d rstd gamma + beta in fp32 (four roundings): |d| rstd |gamma| rel_rstd + e_mu rstd |gamma| + 2^-22 (|d rstd gamma| + |y|);
      * the fp16 store: U |y| + TINY.
    Observed on the MI355X (tests/test_norm_gpu.py): worst error / bound 0.996, signed bias below 3.2e-5 from 320 elements on, 1.0e-4 at one row of 8."""
    xd = x.double()
    c = xd.shape[-1]
    ga, be = gamma.double().to(xd.device), beta.double().to(xd.device)
    mu = xd.mean(-1, keepdim=True)
    d = xd - mu
    var = (d * d).mean(-1, keepdim=True)
    e_mu = c_acc(c) * xd.abs().mean(-1, keepdim=True)
    rstd = (var + eps).rsqrt()
    rel = (c_acc(c) * var + e_mu * e_mu) / (2.0 * (var + eps)) + 2.0 ** -22
    dn = d * rstd * ga
    y = dn + be
    b = dn.abs() * rel + e_mu * rstd * ga.abs() + 2.0 ** -22 * (dn.abs() + y.abs())
    return y, b + U * y.abs() + TINY


def softmax_ref(s, valid=None):
    """fp64 row softmax over the first `valid` columns of the fp16 scores s [rows][cols] (the rest: exactly 0): p_hat, bound
        U p + TINY                        the fp16 store (TINY: most of a long row are fp16 subnormals)
      + (2^-21 + 2^-23 |s - max|) p       __expf = exp2(x log2 e): the argument's rounding scales with |s - max|; exp2, the fp32 sum of the row
                                          and the reciprocal are a few 2^-24 each.
    Observed on the MI355X (tests/test_norm_gpu.py): worst error / bound 0.993.  Signed bias over the largest half of every row: below 2e-5 for 300
    rows of 8 or 40 scale-4 scores; 9.4e-5 for one row of 4096 (half of the kept values are fp16 subnormals: subnormal_bias_allowance; round to
    nearest of the fp64 reference gives the same 9.4e-5) and -1.2e-4 for scores near +-60000 (p = 1 / m for m tied maxima: independent_roundings)."""
    sd = s.double()
    cols = sd.shape[-1]
    valid = cols if valid is None or valid <= 0 else valid
    sv = sd[..., :valid]
    mx = sv.amax(-1, keepdim=True)
    pv = torch.softmax(sv, dim=-1)
    p = torch.zeros_like(sd)
    p[..., :valid] = pv
    bound = torch.full_like(sd, TINY)
    bound[..., :valid] = U * pv + TINY + (2.0 ** -21 + 2.0 ** -23 * (sv - mx).abs()) * pv
    return p, bound


def tapmajor_to_oihw(w, cin):
    """[Cout][9 Cin] (tap-major, channel-minor: the small convolutions' layout) -> [Cout][Cin][3][3]."""
    co = w.shape[0]
    return w.reshape(co, 9, cin).permute(0, 2, 1).reshape(co, cin, 3, 3)


def small_conv_in_ref(x, w, b, scale_sigma=None, pre_w=None, pre_b=None):
    """fp64 reference of small_conv_in_kernel (misc.hip): x fp32 NCHW [n][cin][h][w], w fp16 [Cout][9 cin] tap-major, b fp16 -> y_hat
    [n h w][Cout], bound.  The kernel's stated intermediate roundings are mirrored:
      * v = half(x * inscale), inscale = 1 / sqrt(sigma^2 + 1) in fp32 (1 without scale_sigma: then v = half(x), reproduced exactly).  A
        one-ulp difference of inscale between the device and this mirror can flip the fp16 rounding of an input: e_v = U |v| with scale_sigma;
      * the 1x1 pre-conv t = half(pre_b + pre_w v) (fp32 on the device, fp64 here: the rounding of t can flip): e_t = |pre_w| e_v + U |t|;
        it applies inside the image only — the 3x3 taps outside it read zeros, not pre_b;
      * the input-side error reaches the output as im2col(e) |w|^T; accumulation from the bias in fp32: c_acc(9 cin) (absdot + |b|);
      * the fp16 store: U |y| + TINY.
    Observed on the MI355X (tests/test_small_kernels_gpu.py): worst error / bound 0.994, signed bias below 1e-5 from 2000 elements on, 6.8e-5 at 72 elements."""
    n, cin, h, wd = x.shape
    if scale_sigma is not None:
        sg = scale_sigma.float().to(x.device)
        inscale = 1.0 / torch.sqrt(sg * sg + 1.0)
        v = (x.float() * inscale.reshape(n, 1, 1, 1)).half()
        e = U * v.double().abs()
    else:
        v = x.float().half()
        e = torch.zeros_like(v, dtype=torch.float64)
    vd = v.double()
    if pre_w is not None:
        pw, pb = pre_w.double().to(x.device), pre_b.double().to(x.device)
        t = torch.einsum("oc,nchw->nohw", pw, vd) + pb.reshape(1, -1, 1, 1)
        th = t.half()
        e = torch.einsum("oc,nchw->nohw", pw.abs(), e) + U * th.double().abs()
        vd = th.double()
    wo = tapmajor_to_oihw(w.to(x.device), cin)
    wm = wo.double().reshape(wo.shape[0], -1)
    cols = im2col(vd.permute(0, 2, 3, 1), 3)
    ecols = im2col(e.permute(0, 2, 3, 1), 3)
    bd = b.double().to(x.device)
    y = cols @ wm.t() + bd
    absdot = cols.abs() @ wm.abs().t()
    bound = ecols @ wm.abs().t() + c_acc(9 * cin) * (absdot + bd.abs()) + U * y.abs() + TINY
    return y, bound


def _fp16_ulp(a):
    """Spacing of the fp16 numbers around |a| (the larger one at a power of two)."""
    _, e = torch.frexp(a.abs().clamp_min(2.0 ** -30))
    return torch.pow(2.0, (e - 11).double()).clamp_min(2.0 ** -24)


def small_conv_out_ref(x, w, b, mode, x_in=None, sigma=None, in_mod=0):
    """fp64 reference of small_conv_out_kernel (misc.hip): x fp16 NHWC, w fp16 [Cout][9 Cin] tap-major -> (y_hat, bound) in the layout the
    kernel writes (mode 1: [n h w][Cout]; modes 0, 2: NCHW [n][Cout][h][w]).  v = conv + b: packed fp16 dot products accumulated in fp32 per lane,
    a shuffle tree and the bias add:  e_v = c_acc(9 Cin) (absdot + |b|) + 2^-23 |v|.  No fp16 store: the outputs are fp32.
      mode 2: v.                                                       bound e_v
      mode 1: clamp((v + 1) / 2, 0, 1) (1-Lipschitz).                   bound e_v / 2 + 2^-23 (|v| + 1) / 2
      mode 0: x_in - eps sigma with eps = half(v), mirrored as half(v_hat): the device's eps is the same fp16 number unless v_hat lies within e_v
              of a rounding boundary, where it may be the neighbour: bound = sigma ulp16(v) there, + 2^-23 (|x_in| + 2 |eps sigma|) everywhere.
              Where e_v >= ulp16(v) / 2 (v near zero: the grid is finer than the accumulation error) it may be several numbers away: bound =
              sigma ((1 + 2^-11) e_v + 1.5 ulp16(v)) there.  (The one-step bound alone put 2 to 5 of the 2-5e5 outputs of a full-width UNet
              step outside, all with |v| of 1e-4 — tests/test_unet_chain_full_gpu.py; mode 2 held the same v inside e_v.)
    Observed on the MI355X (tests/test_small_kernels_gpu.py): worst error / bound 0.20 (mode 2), 0.16 (mode 1), 1.000 (mode 0: where eps may be the
    neighbouring fp16 number it sometimes is — the bound there IS that step; 0.45 elsewhere), signed bias below 3e-7."""
    n, h, wd, cin = x.shape
    co = w.shape[0]
    cols = im2col(x, 3)
    wm = tapmajor_to_oihw(w.to(x.device), cin).double().reshape(co, -1)
    y = cols @ wm.t()
    absdot = cols.abs() @ wm.abs().t()
    bd = b.double().to(x.device)
    v = y + bd
    e_v = c_acc(9 * cin) * (absdot + bd.abs()) + 2.0 ** -23 * v.abs() + 1e-30
    nchw = lambda t: t.reshape(n, h, wd, co).permute(0, 3, 1, 2)
    if mode == 2:
        return nchw(v), nchw(e_v)
    if mode == 1:
        return ((v + 1.0) * 0.5).clamp(0.0, 1.0), 0.5 * e_v + 2.0 ** -24 * (v.abs() + 1.0)
    eps = v.half().double()
    ulp = torch.maximum(_fp16_ulp(v), _fp16_ulp(eps))
    flip = (0.5 * ulp - (v - eps).abs()) <= e_v
    # how far the device's eps may lie from the mirror's where it may differ at all: one step of the fp16 grid while e_v < ulp / 2 (two reals
    # closer than half a spacing round to the same or to neighbouring numbers); from there on — a v near zero, where the grid is finer than
    # the accumulation error: |v| < 2^-14 has steps of 2^-24 — several steps: |v_dev - v_hat| <= e_v, the mirror's rounding ulp / 2, the
    # device's max(U |v_dev|, 2^-25) <= ulp + U e_v
    eps_err = torch.where(e_v < 0.5 * ulp, ulp, (1.0 + U) * e_v + 1.5 * ulp)
    idx = torch.arange(n, device=x.device) % (in_mod if in_mod > 0 else n)
    sg = sigma.double().to(x.device)[idx].reshape(n, 1, 1, 1)
    xi = x_in.double().to(x.device)[idx]
    out = xi - nchw(eps) * sg
    bound = nchw(flip.double() * eps_err) * sg.abs() + 2.0 ** -23 * (xi.abs() + 2.0 * (nchw(eps) * sg).abs()) + 1e-30
    return out, bound


def small_pointwise_ref(x, w, b):
    """fp64 out [n][C][hw] = b + w x of x fp16 [n][hw][8] (small_pointwise_kernel: fp32 chain of 8, rounded to fp16, stored as fp32):
    bound U |y| + c_acc(8) (absdot + |b|) + TINY.
    Observed on the MI355X: worst error / bound 0.998, signed bias 1.6e-7 at 2.4e6 elements."""
    xd, wd, bd = x.double(), w.double().to(x.device), b.double().to(x.device)
    y = xd @ wd.t() + bd
    bound = U * y.abs() + c_acc(8) * (xd.abs() @ wd.abs().t() + bd.abs()) + TINY
    return y.transpose(1, 2), bound.transpose(1, 2)


def vae_out_finish_ref(t8, cout):
    """fp64 clamp((v + 1) / 2, 0, 1) of the first cout columns of t8 fp16 [npix][8]: one fp32 add (the halving is exact): bound 2^-24 (|v| + 1).
    Observed on the MI355X: worst error / bound 0.50, signed bias 2e-13."""
    v = t8.double().reshape(-1, 8)[:, :cout]
    return ((v + 1.0) * 0.5).clamp(0.0, 1.0), 2.0 ** -24 * (v.abs() + 1.0)


def timestep_ref(sigma, log_sigmas, dim, n=None, sigma_mod=0):
    """The timestep lookup and sinusoidal embedding of timestep_embed_kernel (misc.hip) in fp64 from the fp32 sigma and table:
    t [n] (the first-occurrence argmin of |log sigma - log_sigmas|, exact), margin [n] (how far the runner-up VALUE's distance lies above the best:
    a case is well posed for an fp32 logf when this is >> 1e-6), emb_hat [n][dim] = [cos(t f) | sin(t f)], bound:
        U                                   the fp16 store of a value in [-1, 1] (absolute)
      + 2^-23 t f (|x| + 2)                 f = expf(x), x = -ln(1e4) i / half in fp32: x's two roundings make f off by 2^-23 |x| relative, expf and
                                            the product t f another 2^-23 — argument rounding, largest at t = 999 near |x| = 1
      + 2^-22                               cosf / sinf.
    Observed on the MI355X (tests/test_small_kernels_gpu.py): t exact in every case; worst error / bound 0.499 (the store), signed bias below 3.5e-5."""
    sg = sigma.double().flatten()
    n = sg.numel() if n is None else n
    if sigma_mod > 0:
        sg = sg[torch.arange(n, device=sg.device) % sigma_mod]
    tab = log_sigmas.double().flatten().to(sg.device)
    dist = (sg.log().unsqueeze(1) - tab.unsqueeze(0)).abs()              # [n][n_sig]
    t = dist.argmin(dim=1)
    best = dist.gather(1, t.unsqueeze(1))
    other = dist.masked_fill(tab.unsqueeze(0) == tab[t].unsqueeze(1), float("inf"))
    margin = (other.amin(dim=1, keepdim=True) - best).flatten()
    half = dim // 2
    xarg = -math.log(10000.0) * torch.arange(half, dtype=torch.float64, device=sg.device) / half
    f = xarg.exp()
    arg = t.double().unsqueeze(1) * f.unsqueeze(0)
    emb = torch.cat([arg.cos(), arg.sin()], dim=1)
    b = U + 2.0 ** -23 * arg * (xarg.abs().unsqueeze(0) + 2.0) + 2.0 ** -22
    return t, margin, emb, torch.cat([b, b], dim=1)


def mlp_out_fold_ref(wpo, w2, b2, bpo):
    """fp64 W' [C][5C] = [Wpo W2 | Wpo] and b' = Wpo b2 + bpo from the fp16 weights (mlp_out_fold_kernel: fp32 chains of C, one rounding):
    (w_hat, w_bound, b_hat, b_bound) with  U |w'| + c_acc(C) sum|Wpo||W2| + TINY;  the identity columns [4C, 5C) are copies: bound 1e-300 there
    (any difference fails; the test also compares them bitwise).
    Observed on the MI355X (tests/test_small_kernels_gpu.py): worst error / bound 0.993 (W'), 0.985 (b'), signed bias 6.4e-7 (W'), 2.2e-5 (b', 64 elements)."""
    a, m = wpo.double(), w2.double()
    c = a.shape[0]
    prod = a @ m
    pb = U * prod.abs() + c_acc(c) * (a.abs() @ m.abs()) + TINY
    bh = a @ b2.double() + bpo.double()
    bb = U * bh.abs() + c_acc(c) * (a.abs() @ b2.double().abs() + bpo.double().abs()) + TINY
    return torch.cat([prod, a], dim=1), torch.cat([pb, torch.full_like(a, 1e-300)], dim=1), bh, bb


def ln_fold_ref(w, gamma, beta, bias=None):
    """fp64 W' = W diag(gamma) and b' = bias + W beta from the fp16 inputs (ln_fold_kernel): (w_hat, w_bound, b_hat, b_bound).
    W': an fp16 x fp16 product is exact in fp32, so its one rounding is U |w'| + TINY;  b': U |b'| + c_acc(K) (sum|W||beta| + |bias|) + TINY.
    wsum is checked against the DEVICE's rounded W' (wsum_ref).
    Observed on the MI355X (tests/test_small_kernels_gpu.py): W' bitwise half(w gamma) (error / bound 0.996, bias 1.6e-6); b' 0.963, bias 3.3e-5 at 192
    elements; wsum 0.067 of its bound."""
    wd, ga, be = w.double(), gamma.double(), beta.double()
    k = wd.shape[1]
    wh = wd * ga
    b0 = torch.zeros(wd.shape[0], dtype=torch.float64, device=w.device) if bias is None else bias.double()
    bh = b0 + wd @ be
    bb = U * bh.abs() + c_acc(k) * (wd.abs() @ be.abs() + b0.abs()) + TINY
    return wh, U * wh.abs() + TINY, bh, bb


def wsum_ref(w_out):
    """fp64 row sums of the device's fp16 W' and the bound of their fp32 sum: c_acc(K) sum|W'| (+ 1e-30: an all-zero row is exact)."""
    wd = w_out.double()
    return wd.sum(-1), c_acc(wd.shape[1]) * wd.abs().sum(-1) + 1e-30


# ------------------------------------------------------------------ a ResBlock half as the UNet executor runs it (tests/test_unet_chain_gpu.py)

def gn_silu_conv_ref(x, gamma, beta, eps, w_oihw, bias, x2=None, rowvec=None, residual=None, skip=None):
    """fp64 conv3x3(SiLU(GroupNorm32(cat(x, x2))); w) + bias (+ rowvec per image) (+ residual) of NHWC fp16 x [n][h][w][C1], x2 [n][h][w][C2], and
    with skip = (s1, s2 or None, wskip [Cout][SC], bskip) the 1x1 convolution of the RAW sources cat(s1, s2) as a second K segment
    (ResBlock1's skip_connection folded into out_layers, LD.py:5267): y_hat [n h w][Cout], bound.
    A composition of references this module already has, nothing new in it:
      * the normalised, activated operand a = SiLU(GN(x)) and ITS element bound e_a from groupnorm_ref (fp32 statistics — a producer's partials
        are fp32 sums of the same fp16 values — the fp32 affine map and SiLU, ONE fp16 rounding: the store of the two-pass route, the halo
        loader's conversion where the norm is fused);
      * the contraction over columns [im2col(a) | s1 | s2] against [w | wskip] with bias b + bskip, by epilogue_ref with K = 9 C + SC, as
        test_routes_gpu.py's skip and GroupNorm routes build it; the operand's error enters as extra = im2col(e_a) |w|^T (the raw skip columns
        carry none), in place of those routes' (2^-11 + 1e-5) |a| |w|^T: the same rounding, with the statistics' share taken from groupnorm_ref's
        model, cancellation term included, instead of a constant."""
    n, h, wd = x.shape[0], x.shape[1], x.shape[2]
    a, e_a = groupnorm_ref(x, x2, gamma, beta, eps, True)
    C = a.shape[-1]
    cout = w_oihw.shape[0]
    cols = im2col(a.reshape(n, h, wd, C), 3)
    ecols = im2col(e_a.reshape(n, h, wd, C), 3)
    wm = w_oihw.double().reshape(cout, -1)
    extra = ecols @ wm.abs().t()
    b = None if bias is None else bias.double()
    if skip is not None:
        s1, s2, wskip, bskip = skip
        sk = (s1 if s2 is None else torch.cat([s1, s2], dim=-1)).double()
        cols = torch.cat([cols, sk.reshape(-1, sk.shape[-1])], dim=1)
        wm = torch.cat([wm, wskip.double().reshape(cout, -1)], dim=1)
        b = (0.0 if b is None else b) + bskip.double()
    rv = None if rowvec is None else rowvec.double().repeat_interleave(h * wd, dim=0)
    res = None if residual is None else residual.reshape(-1, cout)
    return epilogue_ref(cols @ wm.t(), cols.abs() @ wm.abs().t(), wm.shape[1], b, res, extra=extra, rowvec=rv)


# ------------------------------------------------------------------ the end convolutions of the upscaler and the preview decoder (esrgan.hip, taesd.hip)
# Weights are fp16 [Cout][9 Cin], tap-major and channel-minor, as the kernels read them; results [n h w][Cout].

def _end_conv(a, w, b, cin):
    """fp64 conv3x3 (pad 1) of a [n][h][w][>= cin] + b: (pre, sum |a w|) as [n h w][Cout]."""
    cols = im2col(a[..., :cin], 3)
    wm = tapmajor_to_oihw(w.to(a.device), cin).double().reshape(w.shape[0], -1)
    return cols @ wm.t() + b.double().to(a.device), cols.abs() @ wm.abs().t(), wm


def esrgan_first_ref(x, w, b):
    """fp64 reference of esrgan_first_kernel: x fp32 NHWC [n][h][w][3], rounded to fp16 once (the kernel's own rounding, reproduced exactly: no
    allowance), K = 27 fp32 chain from the bias, one fp16 store:  U |y| + c_acc(27) sum|a w| + 2^-23 |pre| + TINY.
    Observed on the MI355X (tests/test_end_convs_gpu.py): worst error / bound 0.993 (the store), signed bias below 5e-6; the fp32 emulation 0.994."""
    pre, absdot, _ = _end_conv(x.half().double(), w, b, 3)
    return pre, U * pre.abs() + c_acc(27) * absdot + 2.0 ** -23 * pre.abs() + TINY


TANH_FP32_REL = 2.0 ** -21      # 3 tanhf(x / 3) against 3 tanh(x / 3): the quotient, tanhf within two ulps, the product


def taesd_clamp_ref(x):
    """a = round_fp16(3 tanh(x / 3)) with tanh in fp64, and what the kernel's fp32 tanhf may change of it: where the fp64 value lies within
    TANH_FP32_REL |t| of a rounding boundary of fp16 the device's operand may be the neighbouring fp16 number — one fp16 ulp there, 0 elsewhere."""
    t = 3.0 * torch.tanh(x.double() / 3.0)
    a = t.half().double()
    ulp = torch.maximum(_fp16_ulp(t), _fp16_ulp(a))
    flip = (0.5 * ulp - (t - a).abs()) <= TANH_FP32_REL * t.abs()
    return a, flip.double() * ulp * (t != 0).double()


def taesd_first_ref(x, w, b):
    """fp64 reference of taesd_first_kernel: latent fp32 NHWC [n][h][w][4] -> relu(conv(a) + b), a = taesd_clamp_ref(x); K = 36:
        U |y| + c_acc(36) sum|a w| + im2col(e_a) |w|^T + 2^-23 |pre| + TINY      (ReLU has Lipschitz constant 1).
    Observed on the MI355X (tests/test_end_convs_gpu.py): worst error / bound 0.991 (the store), signed bias over the positive outputs below 9e-6;
    the fp32 emulation 0.995."""
    a, e_a = taesd_clamp_ref(x)
    pre, absdot, wm = _end_conv(a, w, b, 4)
    y = pre.clamp_min(0.0)
    return y, U * y.abs() + c_acc(36) * absdot + im2col(e_a, 3) @ wm.abs().t() + 2.0 ** -23 * pre.abs() + TINY


def esrgan_last_ref(x, w, b):
    """fp64 reference of esrgan_last_kernel: the first 64 channels of x fp16 NHWC (any pitch) -> [n h w][3] fp32, K = 576 as packed fp16 dot
    products accumulated in fp32 from the bias; no fp16 rounding anywhere:  c_acc(576) sum|a w|  (+ 1e-30: an all-zero patch returns the bias).
    Observed on the MI355X (tests/test_end_convs_gpu.py): worst error / bound 0.59, signed bias below 7e-8; the fp32 emulation 0.48."""
    pre, absdot, _ = _end_conv(x.double(), w, b, 64)
    return pre, c_acc(576) * absdot + 1e-30


def taesd_last_ref(x, w, b):
    """fp64 reference of taesd_last_kernel's fp32 output d = (v - 0.5) * 2: the doubled bound of esrgan_last_ref plus the fp32 subtraction
    (the doubling is exact): 2 c_acc(576) sum|a w| + 2^-23 |d|.  Also the image value floor(clip(255 (d + 1) / 2, 0, 255)) of the fp64 d.
    Observed on the MI355X (tests/test_end_convs_gpu.py): worst error / bound 0.62, signed bias below 1.1e-7; every image byte equal to the truncation of
    the device's own d and within one count of the fp64 byte."""
    pre, absdot, _ = _end_conv(x.double(), w, b, 64)
    d = (pre - 0.5) * 2.0
    img = (255.0 * ((d + 1.0) * 0.5)).clamp(0.0, 255.0).floor()
    return d, 2.0 * c_acc(576) * absdot + 2.0 ** -23 * d.abs() + 1e-30, img


# ------------------------------------------------------------------ tiled_scale's blend (esrgan.hip: tile_blend_kernel, tile_divide_kernel)

def tile_blend_ref(oh, ow, c, tiles, out0=None, div0=None):
    """fp64 accumulation of `tiles` = [(ps [th][tw][c], my [th], mx [tw], y0, x0), ...] in the given order into out [oh][ow][c] and div [oh][ow]
    (from out0 / div0 or zeros), and the quotient out / div:  (out, b_out, div, b_div, quot, b_quot).  Per tile the kernel rounds m = my mx, then
    ps m, then the sum (or fuses the last two): 2^-23 on each magnitude involved —  b_out += 2^-23 (2 |ps m| + |out|),  b_div += 2^-23 (|m| + |div|).
    The divide: b_out / div + |quot| b_div / div, and one fp32 ulp of the quotient.
    Observed on the MI355X (tests/test_blend_gpu.py): worst error / bound 0.41 (out), 0.44 (div), 0.18 (quotient), 0.49 of one ulp for the divide alone;
    the fp32 emulation 0.33, 0.32, 0.21."""
    out = torch.zeros(oh, ow, c, dtype=torch.float64) if out0 is None else out0.double().clone().cpu()
    div = torch.zeros(oh, ow, dtype=torch.float64) if div0 is None else div0.double().clone().cpu()
    b_out, b_div = torch.zeros_like(out), torch.zeros_like(div)
    for ps, my, mx, y0, x0 in tiles:
        th, tw = ps.shape[0], ps.shape[1]
        m = my.double().cpu().reshape(th, 1) * mx.double().cpu().reshape(1, tw)
        p = ps.double().cpu() * m.unsqueeze(-1)
        sy, sx = slice(y0, y0 + th), slice(x0, x0 + tw)
        out[sy, sx] += p
        div[sy, sx] += m
        b_out[sy, sx] += 2.0 ** -23 * (2.0 * p.abs() + out[sy, sx].abs())
        b_div[sy, sx] += 2.0 ** -23 * (m.abs() + div[sy, sx].abs())
    quot = out / div.unsqueeze(-1)
    b_quot = b_out / div.abs().unsqueeze(-1) + quot.abs() * (b_div / div.abs()).unsqueeze(-1) + 2.0 ** -23 * quot.abs()
    return out, b_out + 1e-30, div, b_div + 1e-30, quot, b_quot + 1e-30


# ------------------------------------------------------------------ bislerp (misc.hip: bislerp_axis_kernel), one axis pass

BISLERP_EPS = 1e-5            # the reference's branch thresholds: dot > 1 - 1e-5 copies a, dot < 1e-5 - 1 lerps (LD.py:455-462)


def bislerp_axis_ref(x, len_new, axis_w):
    """fp64 reference of ONE pass of bislerp (LD.py:429-518) over fp32 NCHW x, taken as exact: the resize of the width (axis_w) or of the height to
    len_new.  -> (y_hat, bound, dot), dot [n][ho][wo] the fp64 cosine of every tap pair (NaN-free: 0 for a zero tap).
    The taps (lo, hi, r) are the oracle's _bilinear_taps in fp32: the tap rule is part of the operation's definition.  Per pair a, b (C-vectors):
        na = |a|, nb = |b|, ua = a / na, ub = b / nb (0 for a zero vector), d = ua . ub, om = acos d, s = sin om, M = na (1 - r) + nb r,
        v = M (ga ua + gb ub), ga = sin((1 - r) om) / s, gb = sin(r om) / s;   d > 1 - 1e-5: v = a;   d < 1e-5 - 1: v = a (1 - r) + b r.
    The branch is chosen by the fp64 d.  Bound, to first order, of the kernel's fp32 evaluation:
      * the fp32 sums: e(sum a b) = c_acc(C) sum|a b|, rel(na) = rel(nb) = c_acc(C) / 2 + 2^-23 (the sum of squares, sqrtf, the reciprocal), so
        e_d = c_acc(C) sum|a b| / (na nb) + |d| (c_acc(C) + 2^-21);
      * om = acosf(d): e_om = e_d / s + 2^-22 om, reaching v through |dv/dom| = M |ga' ua + gb' ub| with
        ga' = ((1 - r) cos((1 - r) om) s - sin((1 - r) om) cos om) / s^2 (gb' likewise with r): COMPUTED, it grows without limit towards the poles;
      * r: pos is one fp32 expression of size up to len_old, so e_r = ulp32(len_old), through
        |dv/dr| = |(nb - na)(ga ua + gb ub) + M om (cos(r om) ub - cos((1 - r) om) ua) / s|;
      * the norms in M and in ua, ub: |v| (rel(na) + rel(nb));
      * the remaining operations, 2^-23 each on the magnitudes they act on: the two sines' arguments and values (2^-22 (|sin| + arg) / s each),
        sinf(om) and the quotient, the products and the sum of v = (wa a + wb b) M: 2^-21 M (|ga ua| + |gb ub|) + 2^-22 |v|;
      * the copy branch is exact (bound 1e-300: any difference fails); the lerp branch has 2^-22 (|a (1 - r)| + |b r|) + |b - a| e_r.
    Observed on the MI355X (tests/test_bislerp_gpu.py): worst error / bound 0.22 (C = 1, 6 x 5 -> 9 x 11), signed bias below 6.1e-6; the oracle's fp32
    run on the same inputs 0.097 (tests/test_errbound_cpu.py)."""
    from oracle import sd15_ref as O
    xd = x.double().cpu()
    n, c, h, w = xd.shape
    len_old = w if axis_w else h
    lo, hi, fr = O._bilinear_taps(len_old, len_new)
    r = fr.double()
    if axis_w:
        a, b = xd[:, :, :, lo], xd[:, :, :, hi]
        r = r.view(1, 1, 1, -1)
    else:
        a, b = xd[:, :, lo, :], xd[:, :, hi, :]
        r = r.view(1, 1, -1, 1)
    ssum = lambda t: t.sum(1, keepdim=True)
    na, nb = ssum(a * a).sqrt(), ssum(b * b).sqrt()
    safe = lambda t: torch.where(t > 0, t, torch.ones_like(t))
    ua, ub = a / safe(na), b / safe(nb)
    d = ssum(ua * ub).clamp(-1.0, 1.0)
    om = torch.acos(d)
    s = torch.sin(om)
    ss = torch.where(s > 0, s, torch.ones_like(s))                     # s = 0 only inside the two branches, which do not use it
    sa, sb, ca, cb = torch.sin((1 - r) * om), torch.sin(r * om), torch.cos((1 - r) * om), torch.cos(r * om)
    ga, gb = sa / ss, sb / ss
    M = na * (1 - r) + nb * r
    v = M * (ga * ua + gb * ub)
    cc = c_acc(c)
    rel_n = 0.5 * cc + 2.0 ** -23
    e_d = cc * ssum((a * b).abs()) / (safe(na) * safe(nb)) + d.abs() * (cc + 2.0 ** -21)
    e_om = e_d / ss + 2.0 ** -22 * om
    dga = ((1 - r) * ca * ss - sa * torch.cos(om)) / (ss * ss)
    dgb = (r * cb * ss - sb * torch.cos(om)) / (ss * ss)
    dv_dom = M * (dga * ua + dgb * ub).abs()
    e_r = 2.0 ** (math.floor(math.log2(len_old)) - 23)
    dv_dr = ((nb - na) * (ga * ua + gb * ub) + M * om * (cb * ub - ca * ua) / ss).abs()
    rest = 2.0 ** -22 * M * (((sa.abs() + (1 - r) * om) * ua.abs() + (sb.abs() + r * om) * ub.abs()) / ss) \
        + 2.0 ** -21 * M * ((ga * ua).abs() + (gb * ub).abs()) + 2.0 ** -22 * v.abs()
    bound = dv_dom * e_om + dv_dr * e_r + 2.0 * rel_n * v.abs() + rest + 1e-30
    same, opp = d > 1.0 - BISLERP_EPS, d < BISLERP_EPS - 1.0
    lerp = a * (1 - r) + b * r
    v = torch.where(same, a, torch.where(opp, lerp, v))
    b_lerp = 2.0 ** -22 * ((a * (1 - r)).abs() + (b * r).abs()) + (b - a).abs() * e_r + 1e-30
    bound = torch.where(same, torch.full_like(bound, 1e-300), torch.where(opp, b_lerp, bound))
    return v, bound, d[:, 0]


def bislerp_dots_clear_of_the_thresholds(dot):
    """The input condition of a bislerp case: no pair's fp64 |dot| inside (1 - 2e-5, 1 - 5e-6), where an fp32 evaluation may take the other branch —
    the reference's own discontinuity."""
    a = dot.abs()
    return not bool(((a > 1.0 - 2e-5) & (a < 1.0 - 5e-6)).any())


# ------------------------------------------------------------------ the samplers' elementwise arithmetic (misc.hip: cfg_combine_kernel, axpby_kernel)

def cfg_combine_ref(den2, cfg):
    """fp64 u + (c - u) cfg of den2 = [u ; c] (fp32): the difference, the product and the sum round once each (the last two may fuse):
    2^-23 (|c - u| |cfg| + |(c - u) cfg| + |out|) — one fp32 ulp per operation on its own magnitude, whatever the cancellation in the sum.
    Observed on the MI355X (tests/test_small_kernels_gpu.py): worst error / bound 0.50 over two laps of the grid; cfg = 0 returns u bit for bit."""
    half = den2.shape[0] // 2
    u, c = den2[:half].double(), den2[half:].double()
    t = (c - u) * cfg
    out = u + t
    return out, 2.0 ** -23 * (2.0 * t.abs() + out.abs()) + 1e-30


def axpby_ref(x, a, y=None, b=0.0, z=None, c=0.0):
    """fp64 a x + b y + c z (y, z optional) of fp32 tensors and fp32 scalars: every product and every partial sum rounds once:
    2^-23 (|a x| + |b y| + |c z| + |a x + b y| + |out|).
    Observed on the MI355X (tests/test_small_kernels_gpu.py): worst error / bound 0.46 in all four pointer arms; a = 1, b = c = 0 leaves x bit for bit."""
    t = float(a) * x.double()
    bound = t.abs()
    if y is not None:
        p = float(b) * y.double()
        t = t + p
        bound = bound + p.abs() + t.abs()
    if z is not None:
        p = float(c) * z.double()
        t = t + p
        bound = bound + p.abs() + t.abs()
    return t, 2.0 ** -23 * bound + 1e-30
