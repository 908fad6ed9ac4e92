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


def signed_bias(y: torch.Tensor, ref: torch.Tensor, floor_frac: float = 1e-3) -> float:
    """s = mean((y - y_hat) sign(y_hat)) / mean(|y_hat|) over the elements with |y_hat| above floor_frac * max|y_hat|."""
    y, ref = y.double().flatten(), ref.double().flatten().to(y.device)
    a = ref.abs()
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
          bias_extra: float = 0.0, floor_frac: float = 1e-3):
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
    s = signed_bias(y, ref, floor_frac)
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


def epilogue_ref(acc, absdot, K, bias=None, residual=None, alpha=1.0, act="none", extra=None, rowvec=None):
    """y_hat and its element bound for y = act(alpha * acc + bias) + residual (act 'geglu': acc / absdot hold [value | gate] halves).
    acc, absdot: fp64 A W^T and |A| |W|^T; `extra`: an fp64 tensor of further input-side error of acc (e.g. a rounded normalised operand)."""
    e_acc = c_acc(K) * absdot * abs(alpha)
    if extra is not None:
        e_acc = e_acc + extra * abs(alpha)
    pre = alpha * acc + (0.0 if bias is None else bias.double())
    e_pre = e_acc + (U + 2.0 ** -23) * ((alpha * acc).abs() + pre.abs())      # the staged fp16 tile (and an fp16 bias add)
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


def im2col(x_nhwc: torch.Tensor, ksize: int, stride: int = 1, out_hw=None) -> torch.Tensor:
    """fp64 im2col of an NHWC fp16 tensor (after an optional nearest resize to out_hw): [n * ho * wo][C * k * k], columns (c, ky, kx) —
    the order of a [Cout][C][k][k] weight reshaped to [Cout][C k k]."""
    x = x_nhwc.permute(0, 3, 1, 2).double()
    if out_hw is not None and tuple(out_hw) != tuple(x.shape[-2:]):
        x = torch.nn.functional.interpolate(x, size=tuple(out_hw), mode="nearest")
    cols = torch.nn.functional.unfold(x, ksize, padding=ksize // 2, stride=stride)     # [n][C k k][L]
    return cols.transpose(1, 2).reshape(-1, cols.shape[1])


def conv_ref(x, w_oihw, bias=None, residual=None, stride=1, out_hw=None, x2=None, rowvec=None):
    """fp64 reference of ld_op_conv (NHWC, pad k // 2) as explicit im2col + matmul on the device: y_hat [n*ho*wo][Cout], bound, (ho, wo)."""
    xin = x if x2 is None else torch.cat([x, x2], dim=-1)
    k = w_oihw.shape[-1]
    cols = im2col(xin, k, stride, out_hw)
    wm = w_oihw.double().reshape(w_oihw.shape[0], -1)
    acc = cols @ wm.t()
    absdot = cols.abs() @ wm.abs().t()
    hv, wv = (x.shape[1], x.shape[2]) if out_hw is None else out_hw
    ho, wo = ((hv - 1) // stride + 1, (wv - 1) // stride + 1) if k == 3 else (hv, wv)
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


def cpu_rows_conv(x, w_oihw, rows, stride=1, out_hw=None, x2=None):
    """CPU fp64 convolution at the sampled output pixels (rows of the [n*ho*wo] result), by explicit patch gathering."""
    xin = (x if x2 is None else torch.cat([x, x2], dim=-1)).cpu()
    n, h, wd, c = xin.shape
    hv, wv = (h, wd) if out_hw is None else out_hw
    k = w_oihw.shape[-1]
    ho, wo = ((hv - 1) // stride + 1, (wv - 1) // stride + 1) if k == 3 else (hv, wv)
    wm = w_oihw.cpu().double()
    out = []
    for r in rows:
        img, pix = divmod(r, ho * wo)
        oy, ox = divmod(pix, wo)
        acc = torch.zeros(wm.shape[0], dtype=torch.float64)
        for ky in range(k):
            for kx in range(k):
                vy, vx = oy * stride + ky - k // 2, ox * stride + kx - k // 2
                if 0 <= vy < hv and 0 <= vx < wv:
                    sy, sx = (vy * h) // hv, (vx * wd) // wv           # nearest resize: source pixel floor(v * in / out)
                    acc += wm[:, :, ky, kx] @ xin[img, sy, sx].double()
        out.append(acc)
    return torch.stack(out)


def attention_ref(q, k, v, heads, causal=False, ones=None):
    """fp64 softmax(q k^T / sqrt(d)) v on the device from the fp16 inputs ([b][L][heads d]) and its element bound:
        2 * 2^-11 |o_hat|                      output rounding + (without the ones column) P's rounding against an unrounded denominator
      + 2^-11 sum p |v - o_hat| / sum p          P rounded to fp16 (RTN: relative 2^-11 per weight)
      + sum p |ds| |v - o_hat| / sum p           Q * scale * log2(e) rounded once: |ds_j| <= 2^-11 scale sum_c |q_c| |k_jc|
      + c_acc(Lk) sum p |v| / sum p + 2^-24     fp32 accumulation of O and the fp32 reciprocal."""
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
    back = lambda t: t.transpose(1, 2).reshape(b, lq, c)
    return back(o), back(bound)
