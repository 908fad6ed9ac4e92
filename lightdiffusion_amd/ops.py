"""Operator-level host mirror of the reference's `operations=` namespace (LD.py:2342-2429) and
`optimized_attention` (LD.py:3966-3988), backed by the HIP library through the C ABI.

Tensors are torch CUDA tensors used as *device memory only*: fp16, channels-last activations
([N,H,W,C] == [N, H*W, C] tokens), weights as the checkpoint stores them.  Every function raises
`LDError` on a non-zero status; none falls back to PyTorch math.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import torch

from ._lib import CONTROL_MAX_SEGMENTS, ERR_SHAPE, F16, F32, LDError, check, lib


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "device-resident contiguous tensors only"
    return t.data_ptr()


def last_kernel() -> str:
    """The kernel instantiations the last operator call on this thread dispatched, in launch order, joined with ';' ("" when it
    dispatched no GEMM / convolution / attention kernel) — the names of the profile tables."""
    return lib().ld_op_last_kernel().decode()


def last_launches() -> str:
    """EVERY launch of the last operator call on this thread, in launch order and joined with ';', under the names the executors' launch
    tables print (`profile_launches`): the contractions as `last_kernel`, and the norm / boundary launches ("gn_stats_kernel+gn_finalize_kernel",
    "gn_apply_kernel", "timestep_embed_kernel", ...)."""
    return lib().ld_op_last_launches().decode()


_WS = {}


def _ws(nbytes: int, device) -> torch.Tensor:
    """Scratch for split-K partials / GEGLU repack / LN-fold temporaries, cached per (device, stream) and grown on demand: the
    operator seam is also the CLIP path (60+ calls per prompt), so no per-call allocation.  Reuse is stream-ordered — every op
    that takes the buffer runs on the stream the buffer is keyed by and is done with it when the next one starts — so ops
    issued on two streams never share slabs.  Under hipGraph capture nothing is cached: a buffer first grown there would live in
    the graph's private pool (and a cached pointer baked into a graph would race with eager ops), so capture allocates per call.
    The result is always exactly max(nbytes, 256) bytes long, a view of the cached buffer: the kernels size their split over K by the
    scratch they are handed, so an op's route and its bits must not depend on how far earlier ops happened to grow the cache."""
    d = torch.device(device)
    idx = d.index if d.index is not None else torch.cuda.current_device()
    n = max(nbytes, 256)
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(n, dtype=torch.uint8, device=device)
    key = (idx, torch.cuda.current_stream(idx).cuda_stream)
    buf = _WS.get(key)
    if buf is None or buf.numel() < n:
        buf = torch.empty(n, dtype=torch.uint8, device=device)
        _WS[key] = buf
    return buf[:n]


def linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
           act: str = "none", alpha: float = 1.0) -> torch.Tensor:
    """y = act(alpha * x @ weight.T + bias) + residual.  x [..., K] fp16, weight [N, K] fp16 (nn.Linear layout).
    act='geglu': weight/bias rows are [value | gate] as in the checkpoint (LD.py:4508-4515); y has N/2 columns."""
    code = {"none": 0, "silu": 1, "geglu": 2, "quick_gelu": 3}[act]
    K = x.shape[-1]
    N = weight.shape[0]
    M = x.numel() // K
    y = torch.empty(*x.shape[:-1], N // 2 if code == 2 else N, dtype=torch.float16, device=x.device)
    ws = _ws(64 << 20, x.device)
    check(lib().ld_op_linear(_p(x), _p(weight), _p(bias), _p(residual), _p(y), M, N, K, alpha, code, _p(ws), ws.numel(), _stream()),
          "ld_op_linear")
    return y


def linear_ln(x: torch.Tensor, w_prod: torch.Tensor, b_prod: Optional[torch.Tensor], gamma: torch.Tensor, beta: torch.Tensor,
              weight: torch.Tensor, bias: Optional[torch.Tensor], eps: float = 1e-5, residual: Optional[torch.Tensor] = None):
    """The UNet's LayerNorm fold as an operator pair: t = x @ w_prod.T + b_prod (+ residual);  y = LayerNorm(t) @ weight.T + bias with the
    normalisation finished on the GEMM accumulators (no LayerNorm launch, no normalised tensor).  Returns (t, y)."""
    M, C = x.shape
    N = weight.shape[0]
    t = torch.empty(M, C, dtype=torch.float16, device=x.device)
    y = torch.empty(M, N, dtype=torch.float16, device=x.device)
    ws = _ws(2 * N * C + 8 * N + 8 * ((C + 63) // 64) * M + 4096, x.device)
    check(lib().ld_op_linear_ln(_p(x), _p(w_prod), _p(b_prod), _p(residual), _p(gamma), _p(beta), _p(weight), _p(bias), _p(t), _p(y), M, C, N, eps,
                                _p(ws), ws.numel(), _stream()), "ld_op_linear_ln")
    return t, y


def linear_ln_geglu(x: torch.Tensor, w_prod: torch.Tensor, b_prod: Optional[torch.Tensor], gamma: torch.Tensor, beta: torch.Tensor,
                    weight: torch.Tensor, bias: torch.Tensor, eps: float = 1e-5, residual: Optional[torch.Tensor] = None):
    """linear_ln with the GEGLU of FeedForward.net[0] as the consumer: t = x @ w_prod.T + b_prod;  [a | g] = LayerNorm(t) @ weight.T + bias;
    y = a * gelu(g) — the transformer block's MLP input as the executor runs it.  Returns (t, y) with y of width N / 2."""
    M, C = x.shape
    N = weight.shape[0]
    t = torch.empty(M, C, dtype=torch.float16, device=x.device)
    y = torch.empty(M, N // 2, dtype=torch.float16, device=x.device)
    ws = _ws(4 * N * C + 12 * N + 8 * ((C + 63) // 64) * M + 4096, x.device)
    check(lib().ld_op_linear_ln_geglu(_p(x), _p(w_prod), _p(b_prod), _p(residual), _p(gamma), _p(beta), _p(weight), _p(bias), _p(t), _p(y), M, C, N, eps,
                                      _p(ws), ws.numel(), _stream()), "ld_op_linear_ln_geglu")
    return t, y


def repack_conv_weight(w_oihw: torch.Tensor) -> torch.Tensor:
    """[O,I,kh,kw] (fp16/fp32) -> fp16 [O, kh*kw*I] tap-major / channel-minor, the layout the conv kernels read."""
    O, I, kh, kw = w_oihw.shape
    w_oihw = w_oihw.contiguous()
    out = torch.empty(O, kh * kw * I, dtype=torch.float16, device=w_oihw.device)
    if kh == 3:
        check(lib().ld_op_repack_conv(_p(w_oihw), F32 if w_oihw.dtype == torch.float32 else F16, O, I, _p(out), _stream()),
              "ld_op_repack_conv")
    else:
        out.copy_(w_oihw.reshape(O, I))
    return out


FORM_UNET, FORM_VAE = 0, 1      # LD_FORM_*: whose launch a convolution operator reproduces (include/ld_mi355x.h)
_VAE_WS = (96 << 20) + 4096     # the VAE executor's split partials, and room for the operator's alignment


def _conv_out_size(hv, wv, ksize, stride, pad, out_size):
    """(ho, wo) and the (pad, ho, wo) arguments of the C entry points: out_size is only meaningful beside an explicit pad."""
    if pad is None:
        assert out_size is None
        return ((hv - 1) // stride + 1 if ksize == 3 else hv), ((wv - 1) // stride + 1 if ksize == 3 else wv), (-1, 0, 0)
    if out_size is None:
        out_size = ((hv + pad + ksize // 2 - ksize) // stride + 1, (wv + pad + ksize // 2 - ksize) // stride + 1)
    ho, wo = out_size
    # every tap row / column the output reads lies at most one zero row / column outside the image (the loader's bounds check supplies those)
    assert 1 <= ho and (ho - 1) * stride - pad + ksize - 1 <= hv and 1 <= wo and (wo - 1) * stride - pad + ksize - 1 <= wv, "output larger than the padded image"
    return ho, wo, (pad, ho, wo)


def conv2d(x: torch.Tensor, w_packed: torch.Tensor, bias: Optional[torch.Tensor], ksize: int = 3, stride: int = 1,
           x2: Optional[torch.Tensor] = None, out_hw: Optional[tuple] = None, rowvec: Optional[torch.Tensor] = None,
           residual: Optional[torch.Tensor] = None, pad: Optional[int] = None, out_size: Optional[tuple] = None, n_valid: int = 0, ldc: int = 0,
           form: int = FORM_UNET) -> torch.Tensor:
    """NHWC conv (pad ksize//2) over the channel concat of x [N,H,W,C1] and optional x2 [N,H,W,C2];
    `out_hw` first resizes the input nearest-neighbour (Upsample1, LD.py:5141-5152); rowvec [N,Cout] is added per image.
    pad / out_size: zeros above and left of the image and the output's (ho, wo) — the zeros below and right follow from it (pad=0 at stride 2:
    the VAE encoder's Downsample, F.pad (0, 1, 0, 1), LD.py:3514-3528).  n_valid / ldc: only the first n_valid rows of w_packed are read and y
    has ldc columns (the VAE's output convolution on weights zero-padded to 32 rows: n_valid = ldc = 8).  form: FORM_VAE plans the launch under
    the VAE executor's scratch."""
    n, h, w, c1 = x.shape
    c2 = 0 if x2 is None else x2.shape[-1]
    hv, wv = (h, w) if out_hw is None else out_hw
    cout = w_packed.shape[0]
    ho, wo, geom = _conv_out_size(hv, wv, ksize, stride, pad, out_size)
    y = torch.empty(n, ho, wo, ldc or cout, dtype=torch.float16, device=x.device)
    ws = _ws(_VAE_WS if form == FORM_VAE else 192 << 20, x.device)
    check(lib().ld_op_conv(_p(x), c1, _p(x2), c2, n, h, w, hv, wv, stride, ksize, _p(w_packed), _p(bias), _p(rowvec), _p(residual),
                           _p(y), cout, *geom, n_valid, ldc, form, _p(ws), ws.numel(), _stream()), "ld_op_conv")
    return y


def vae_conv_out_takes_halo_tile(c: int, n: int, h: int, w: int, out_ch: int) -> bool:
    """Host only: does the VAE executor run its output convolution [n, h, w, c] -> out_ch on the halo-tile kernel (conv2d on weights padded to
    32 rows with n_valid = ldc = 8 and FORM_VAE, then vae_out_finish) or on small_conv_out (mode 1)?"""
    return bool(lib().ld_op_vae_conv_out_takes_halo_tile(c, n, h, w, out_ch))


def linear_batched(x: torch.Tensor, w: torch.Tensor, M: int, N: int, K: int, batch: int, strides: tuple, lda: int, ldw: int = 0,
                   bias: Optional[torch.Tensor] = None, bias_m: Optional[torch.Tensor] = None, n_valid: int = 0, alpha: float = 1.0) -> torch.Tensor:
    """y [batch, M, N] = alpha * x_b @ w_b[:n_valid].T (+ bias[N]) (+ bias_m[M] along the rows); columns n_valid .. N-1 hold the biases alone.
    x, w: tensors (or views into one) read as [M, lda] / [N, ldw] per batch element at the element strides (sA, sW) = strides (0: shared) — the
    three contractions of the VAE's AttnBlock where no flash kernel takes the width (V^T = Wv g^T + bv, S = Q K^T / sqrt(C), O = P V)."""
    sA, sW = strides
    ldw = ldw or K
    nv = n_valid or N
    assert x.is_cuda and w.is_cuda and x.dtype == w.dtype == torch.float16
    room = lambda t: (t.untyped_storage().nbytes() - t.storage_offset() * 2) // 2          # halfs from the view's first element to the end of its storage
    assert (batch - 1) * sA + (M - 1) * lda + K <= room(x) and (batch - 1) * sW + (nv - 1) * ldw + K <= room(w), "operand smaller than the problem"
    assert bias is None or bias.numel() >= N
    assert bias_m is None or bias_m.numel() >= M
    y = torch.empty(batch, M, N, dtype=torch.float16, device=x.device)
    ws = _ws(_VAE_WS, x.device)
    check(lib().ld_op_linear_batched(x.data_ptr(), lda, w.data_ptr(), ldw, _p(bias), _p(bias_m), _p(y), M, N, K, n_valid, alpha, batch, sA, sW, M * N,
                                     _p(ws), 96 << 20, _stream()), "ld_op_linear_batched")
    return y


def upconv2x_fold(w_packed: torch.Tensor) -> torch.Tensor:
    """The 16 phase-tap matrices of a nearest-2x upsample + 3x3 convolution, from w_packed [O, 9*I] (repack_conv_weight):
    fp16 [4, O, 4*I] = [py*2+px][O][a*2+b][I], sums of the 3x3 taps that fall on one source pixel (fp32 sums, one rounding)."""
    O = w_packed.shape[0]
    I = w_packed.shape[1] // 9
    out = torch.empty(4, O, 4 * I, dtype=torch.float16, device=w_packed.device)
    check(lib().ld_op_upconv2x_fold(_p(w_packed), O, I, _p(out), _stream()), "ld_op_upconv2x_fold")
    return out


def upconv2x(x: torch.Tensor, w_packed: torch.Tensor, w_fold: torch.Tensor, bias: Optional[torch.Tensor], out_hw: Optional[tuple] = None) -> torch.Tensor:
    """Upsample1 (LD.py:5141-5152) as the UNet executor runs it: nearest resize of x [N,H,W,C] to out_hw (default 2H x 2W), then the 3x3
    convolution — on the folded weights (upconv2x_fold) for an exact 2x resize of more than two images, otherwise as conv2d."""
    n, h, w, c = x.shape
    hv, wv = (2 * h, 2 * w) if out_hw is None else out_hw
    cout = w_packed.shape[0]
    y = torch.empty(n, hv, wv, cout, dtype=torch.float16, device=x.device)
    ws = _ws(192 << 20, x.device)
    check(lib().ld_op_upconv2x(_p(x), c, n, h, w, hv, wv, _p(w_packed), _p(w_fold), _p(bias), _p(y), cout, _p(ws), ws.numel(), _stream()),
          "ld_op_upconv2x")
    return y


def conv2d_skip(x: torch.Tensor, w_packed: torch.Tensor, bias: torch.Tensor, s1: torch.Tensor, s2: Optional[torch.Tensor], w_skip: torch.Tensor,
                b_skip: torch.Tensor, rowvec: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ResBlock1's out_layers convolution + its 1x1 skip_connection as one contraction (LD.py:5267, 5273-5287):
    y = conv3x3(x; w_packed) + bias + conv1x1(cat(s1, s2); w_skip) + b_skip.  x [N,H,W,C]; s1 / s2 raw NHWC sources of the same H x W;
    w_skip [Cout, C(s1) + C(s2)] (the checkpoint's [O, I, 1, 1] reshaped)."""
    n, h, w, c = x.shape
    sc1 = s1.shape[-1]
    sc2 = 0 if s2 is None else s2.shape[-1]
    cout = w_packed.shape[0]
    y = torch.empty(n, h, w, cout, dtype=torch.float16, device=x.device)
    ws = _ws(lib().ld_op_conv_skip_ws_bytes(c, sc1, sc2, cout), x.device)
    check(lib().ld_op_conv_skip(_p(x), c, n, h, w, _p(w_packed), _p(bias), _p(s1), sc1, _p(s2), sc2, _p(w_skip), _p(b_skip), _p(rowvec), _p(y), cout,
                                _p(ws), ws.numel(), _stream()), "ld_op_conv_skip")
    return y


def group_norm_silu_conv2d_skip(x: torch.Tensor, gamma: Optional[torch.Tensor], beta: Optional[torch.Tensor], eps: float, w_packed: torch.Tensor,
                                bias: torch.Tensor, s1: torch.Tensor, s2: Optional[torch.Tensor], w_skip: torch.Tensor, b_skip: torch.Tensor,
                                rowvec: Optional[torch.Tensor] = None, partials: bool = False, in_part: Optional[torch.Tensor] = None):
    """A ResBlock's second half as the UNet executor runs it (LD.py:5267, 5273-5287):
    y = conv3x3(SiLU(GroupNorm32(x)); w_packed) + bias + conv1x1(cat(s1, s2); w_skip) + b_skip, the raw skip sources a second K segment of
    the one contraction.  gamma / beta None: x is taken as it is (conv2d_skip).  partials: also return the GroupNorm(32) partial statistics
    the launch wrote for y ([n, chunks, 32, 2] fp32, or None where this shape's kernel writes none), as conv2d_gn_partials.  in_part: the
    partial statistics of x from its producer ([n, chunks, 32, 2]): the GroupNorm skips its statistics pass."""
    import ctypes
    n, h, w, c = x.shape
    sc1 = s1.shape[-1]
    sc2 = 0 if s2 is None else s2.shape[-1]
    cout = w_packed.shape[0]
    y = torch.empty(n, h, w, cout, dtype=torch.float16, device=x.device)
    part = torch.zeros(lib().ld_op_conv_gn_partials_floats(n, h * w), dtype=torch.float32, device=x.device) if partials else None
    chunks = ctypes.c_int(0)
    ws = _ws(lib().ld_op_groupnorm_conv_skip_ws_bytes(c, sc1, sc2, cout, n, h, w), x.device)
    check(lib().ld_op_groupnorm_conv_skip(_p(x), c, n, h, w, _p(gamma), _p(beta), eps, _p(w_packed), _p(bias), _p(s1), sc1, _p(s2), sc2, _p(w_skip),
                                          _p(b_skip), _p(rowvec), _p(y), cout, _p(in_part), 0 if in_part is None else in_part.shape[1], _p(part),
                                          ctypes.byref(chunks) if partials else None, _p(ws), ws.numel(),
                                          _stream()), "ld_op_groupnorm_conv_skip")
    if not partials:
        return y
    return y, (None if chunks.value == 0 else part[: n * chunks.value * 64].view(n, chunks.value, 32, 2))


def conv2d_gn_partials(x: torch.Tensor, w_packed: torch.Tensor, bias: Optional[torch.Tensor], out_hw: Optional[tuple] = None,
                       residual: Optional[torch.Tensor] = None, ksize: int = 3, stride: int = 1, x2: Optional[torch.Tensor] = None,
                       pad: Optional[int] = None, out_size: Optional[tuple] = None, form: int = FORM_UNET):
    """NHWC conv (conv2d's arguments; 3x3 stride 1 by default) that also returns the GroupNorm(32) partial statistics its kernel wrote for the OUTPUT:
    (y, part [n, chunks, 32, 2] fp32 or None when this shape's kernel writes none) — what the executors hand to the next GroupNorm
    (ResBlock1, LD.py:5224-5262; ResnetBlock, LD.py:3560-3576) instead of a statistics pass.  pad / out_size / form: as conv2d; under FORM_VAE
    only the halo tile's epilogue writes statistics (the VAE executor's request), so `part` is None wherever another kernel takes the shape."""
    import ctypes
    n, h, w, c = x.shape
    c2 = 0 if x2 is None else x2.shape[-1]
    hv, wv = (h, w) if out_hw is None else out_hw
    cout = w_packed.shape[0]
    ho, wo, geom = _conv_out_size(hv, wv, ksize, stride, pad, out_size)
    y = torch.empty(n, ho, wo, cout, dtype=torch.float16, device=x.device)
    part = torch.zeros(lib().ld_op_conv_gn_partials_floats(n, ho * wo), dtype=torch.float32, device=x.device)
    chunks = ctypes.c_int(0)
    ws = _ws(_VAE_WS if form == FORM_VAE else 192 << 20, x.device)
    check(lib().ld_op_conv_gn_partials(_p(x), c, _p(x2), c2, n, h, w, hv, wv, stride, ksize, _p(w_packed), _p(bias), _p(residual), _p(y), cout, *geom, 0, 0,
                                       form, _p(part), ctypes.byref(chunks), _p(ws), ws.numel(), _stream()), "ld_op_conv_gn_partials")
    if chunks.value == 0:
        return y, None
    return y, part[: n * chunks.value * 64].view(n, chunks.value, 32, 2)


def group_norm_silu_conv2d(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, w_packed: torch.Tensor,
                           bias: Optional[torch.Tensor], x2: Optional[torch.Tensor] = None, rowvec: Optional[torch.Tensor] = None,
                           residual: Optional[torch.Tensor] = None, partials: bool = False, in_part: Optional[torch.Tensor] = None,
                           form: int = FORM_UNET):
    """conv3x3(SiLU(GroupNorm32(cat(x, x2)))) + rowvec + residual on NHWC fp16 — ResBlock1.in_layers / out_layers (LD.py:5224-5262)
    as ONE operator: on the halo-tile convolution kernel the normalisation happens inside the conv's A operand.  in_part: the GroupNorm
    partial statistics of x from its producer ([n, chunks, 32, 2]; x2 must be None): no statistics pass.  partials: returns (y, the partial
    statistics the launch wrote for y, or None where this shape's kernel writes none), as conv2d_gn_partials.  form: FORM_VAE for a
    ResnetBlock half (LD.py:3560-3576) as the VAE executor launches it."""
    import ctypes
    n, h, w, c1 = x.shape
    c2 = 0 if x2 is None else x2.shape[-1]
    cout = w_packed.shape[0]
    y = torch.empty(n, h, w, cout, dtype=torch.float16, device=x.device)
    part = torch.zeros(lib().ld_op_conv_gn_partials_floats(n, h * w), dtype=torch.float32, device=x.device) if partials else None
    chunks = ctypes.c_int(0)
    ws = _ws(lib().ld_op_groupnorm_conv_ws_bytes(c1, c2, n, h, w, cout), x.device)
    check(lib().ld_op_groupnorm_conv(_p(x), c1, _p(x2), c2, n, h, w, _p(gamma), _p(beta), eps, _p(w_packed), _p(bias), _p(rowvec), _p(residual),
                                     _p(y), cout, _p(in_part), 0 if in_part is None else in_part.shape[1], _p(part),
                                     ctypes.byref(chunks) if partials else None, form, _p(ws), ws.numel(), _stream()), "ld_op_groupnorm_conv")
    if not partials:
        return y
    return y, (None if chunks.value == 0 else part[: n * chunks.value * 64].view(n, chunks.value, 32, 2))


def conv_takes_skip_segment(c: int, n: int, h: int, w: int, cout: int) -> bool:
    """Host only: does the UNet executor fold a ResBlock's 1x1 skip_connection into out_layers' 3x3 convolution [n, h, w, c] -> cout
    (group_norm_silu_conv2d_skip), or run it as a launch of its own in front (conv2d with ksize 1, then the residual)?"""
    return bool(lib().ld_op_conv_takes_skip_segment(c, n, h, w, cout))


def group_norm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, silu: bool = False,
               x2: Optional[torch.Tensor] = None) -> torch.Tensor:
    """GroupNorm(32) (+SiLU) over the channel concat of NHWC x and x2, written as one contiguous NHWC tensor."""
    n, c1 = x.shape[0], x.shape[-1]
    hw = x.numel() // (n * c1)
    c2 = 0 if x2 is None else x2.shape[-1]
    y = torch.empty(*x.shape[:-1], c1 + c2, dtype=torch.float16, device=x.device)
    ws = _ws(lib().ld_op_groupnorm_ws_bytes(n, hw), x.device)
    check(lib().ld_op_groupnorm(_p(x), c1, _p(x2), c2, n, hw, _p(gamma), _p(beta), eps, int(silu), _p(y), _p(ws), _stream()),
          "ld_op_groupnorm")
    return y


def layer_norm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    c = x.shape[-1]
    y = torch.empty_like(x)
    check(lib().ld_op_layernorm(_p(x), _p(gamma), _p(beta), _p(y), x.numel() // c, c, eps, _stream()), "ld_op_layernorm")
    return y


def clip_embed(ids, table: torch.Tensor, pos: torch.Tensor, extra: Optional[torch.Tensor] = None):
    """CLIP's input stage (CLIPEmbeddings, LD.py:4394-4410): out[b, l] = fp16(float(row(ids[b][l])) + float(pos[l])), fp16 [B, L, h].
    `ids`: [B][L] host integers (a list or a tensor); `table` fp16 [V, h], resident; `extra` fp32 [E, h]: the prompt's textual-inversion
    vectors.  row(id) = table[id] below V-1, extra[id - (V-1)] from V-1 to V-2+E, table[V-1] (EOS) at V-1+E.  The ids are range-checked here,
    on the host, before they are uploaded (ValueError); nothing of V rows is allocated.  Returns (out, the ids as an int32 device tensor)."""
    host = torch.as_tensor(ids).to("cpu", torch.int64)
    if host.dim() != 2 or host.numel() == 0:
        raise ValueError(f"clip_embed: ids must be [B][L], got shape {tuple(host.shape)}")
    (V, h), E = table.shape, 0 if extra is None else extra.shape[0]
    B, L = host.shape
    lo, hi = int(host.min()), int(host.max())
    if lo < 0 or hi > V - 1 + E:
        raise ValueError(f"clip_embed: token id {lo if lo < 0 else hi} outside [0, {V - 1 + E}] (vocabulary {V}, {E} custom vectors)")
    assert table.dtype == torch.float16 and pos.dtype == torch.float16 and pos.shape[1] == h, "fp16 token and position tables of one width"
    if extra is not None:
        assert extra.dtype == torch.float32 and extra.shape[1] == h, "custom vectors are fp32 [E, h]"
    if L > pos.shape[0]:
        raise LDError(ERR_SHAPE, f"ld_op_clip_embed: {L} tokens per row, the position table has {pos.shape[0]}")
    dev = host.to(torch.int32).to(table.device)
    out = torch.empty(B, L, h, dtype=torch.float16, device=table.device)
    check(lib().ld_op_clip_embed(_p(dev), _p(table), _p(extra) if E else None, _p(pos), _p(out), B, L, V, E, h, _stream()), "ld_op_clip_embed")
    return out, dev


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, causal: bool = False) -> torch.Tensor:
    """optimized_attention(q, k, v, heads) of LD.py:3966-3978: q [b,Lq,heads*d], k/v [b,Lk,heads*d] -> [b,Lq,heads*d].
    (The executor never materialises V^T like this — its projection GEMM writes V^T directly.)"""
    b, lq, c = q.shape
    lk = k.shape[1]
    d = c // heads
    lkp = (lk + 7) // 8 * 8
    vt = torch.zeros(b, c, lkp, dtype=torch.float16, device=q.device)
    vt[:, :, :lk] = v.transpose(1, 2)
    o = torch.empty_like(q)
    check(lib().ld_op_attention(_p(q), c, _p(k.contiguous()), c, _p(vt), lkp, _p(o), c, b, heads, lq, lk, d, 1.0 / math.sqrt(d), int(causal), _stream()),
          "ld_op_attention")
    return o


def attention_vt(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, heads: int) -> torch.Tensor:
    """attention() on operands projected once per context (context_kv): k [b, Lk, heads*d], vt [b, heads*d, Lk padded to 8] = V transposed."""
    b, lq, c = q.shape
    lk = k.shape[1]
    o = torch.empty_like(q)
    d = c // heads
    check(lib().ld_op_attention(_p(q), c, _p(k), c, _p(vt), vt.shape[2], _p(o), c, b, heads, lq, lk, d, 1.0 / math.sqrt(d), 0, _stream()),
          "ld_op_attention")
    return o


def attention_qkv(qkv: torch.Tensor, heads: int, causal: bool = False) -> torch.Tensor:
    """Self-attention on a fused projection qkv [b, L, 3*heads*d] = [q | k | v] (how the UNet executor runs attn1 of
    BasicTransformerBlock, LD.py:4117-4162): V is read row-major, no transposed copy."""
    b, l, c3 = qkv.shape
    c = c3 // 3
    d = c // heads
    o = torch.empty(b, l, c, dtype=torch.float16, device=qkv.device)
    base = qkv.data_ptr()
    check(lib().ld_op_attention_rowv(base, c3, base + 2 * c, c3, base + 4 * c, c3, _p(o), c, b, heads, l, l, d, 1.0 / math.sqrt(d), int(causal),
                                     _stream()), "ld_op_attention_rowv")
    return o


def attention_rowv(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, causal: bool = False) -> torch.Tensor:
    """attention() with V handed over row-major [b, Lk, heads*d]."""
    b, lq, c = q.shape
    lk = k.shape[1]
    d = c // heads
    o = torch.empty_like(q)
    check(lib().ld_op_attention_rowv(_p(q), c, _p(k.contiguous()), c, _p(v.contiguous()), c, _p(o), c, b, heads, lq, lk, d, 1.0 / math.sqrt(d), int(causal),
                                     _stream()), "ld_op_attention_rowv")
    return o


def softmax_rows_(s: torch.Tensor) -> torch.Tensor:
    cols = s.shape[-1]
    check(lib().ld_op_softmax_rows(_p(s), s.numel() // cols, cols, _stream()), "ld_op_softmax_rows")
    return s


def timestep_embed(sigma: torch.Tensor, log_sigmas: torch.Tensor, dim: int):
    n = sigma.numel()
    out = torch.empty(n, dim, dtype=torch.float16, device=sigma.device)
    t = torch.empty(n, dtype=torch.float32, device=sigma.device)
    check(lib().ld_op_timestep_embed(_p(sigma), _p(log_sigmas), log_sigmas.numel(), n, dim, _p(out), _p(t), _stream()),
          "ld_op_timestep_embed")
    return out, t


# ------------------------------------------------------------------ the norm, boundary-convolution and fold kernels on their own
# (the seam of tests/test_norm_gpu.py and tests/test_small_kernels_gpu.py; the executors call the launchers directly)
def softmax_rows_ld_(s: torch.Tensor, cols: int, valid: int = 0) -> torch.Tensor:
    """In-place row softmax over the first `cols` columns of s [rows][ld]; columns valid .. cols-1 become zeros, cols .. ld-1 stay."""
    ld = s.shape[-1]
    check(lib().ld_op_softmax_rows_ld(_p(s), s.numel() // ld, cols, ld, valid, _stream()), "ld_op_softmax_rows_ld")
    return s


def _gn_dims(x, x2):
    n, c1 = x.shape[0], x.shape[-1]
    return n, c1, 0 if x2 is None else x2.shape[-1], x.numel() // (n * c1)


def group_norm_stats(x: torch.Tensor, x2: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The statistics pass alone: partial (sum, sum of squares) [n][chunks][32][2] fp32."""
    n, c1, c2, hw = _gn_dims(x, x2)
    part = torch.empty(n, lib().ld_op_groupnorm_chunks(n, hw), 32, 2, dtype=torch.float32, device=x.device)
    check(lib().ld_op_groupnorm_stats(_p(x), c1, _p(x2), c2, n, hw, _p(part), _stream()), "ld_op_groupnorm_stats")
    return part


def group_norm_from_partials(x: torch.Tensor, part: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, silu: bool = False,
                             x2: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The apply pass alone over a producer's partials [n][pstat][32][2]."""
    n, c1, c2, hw = _gn_dims(x, x2)
    y = torch.empty(*x.shape[:-1], c1 + c2, dtype=torch.float16, device=x.device)
    check(lib().ld_op_groupnorm_from_partials(_p(x), c1, _p(x2), c2, n, hw, _p(gamma), _p(beta), eps, int(silu), _p(y), _p(part), part.shape[1],
                                              _stream()), "ld_op_groupnorm_from_partials")
    return y


def group_norm_scale_shift(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, x2: Optional[torch.Tensor] = None,
                           part: Optional[torch.Tensor] = None):
    """(scale, shift) [n][C] fp32 of y = x * scale + shift; part: a producer's partials [n][pstat][32][2] (None: the statistics pass runs)."""
    n, c1, c2, hw = _gn_dims(x, x2)
    scale = torch.empty(n, c1 + c2, dtype=torch.float32, device=x.device)
    shift = torch.empty_like(scale)
    ws = part if part is not None else _ws(lib().ld_op_groupnorm_ws_bytes(n, hw), x.device)
    check(lib().ld_op_groupnorm_scale_shift(_p(x), c1, _p(x2), c2, n, hw, _p(gamma), _p(beta), eps, _p(ws), 0 if part is None else part.shape[1],
                                            _p(scale), _p(shift), _stream()), "ld_op_groupnorm_scale_shift")
    return scale, shift


def small_conv_in(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, scale_sigma: Optional[torch.Tensor] = None,
                  pre_w: Optional[torch.Tensor] = None, pre_b: Optional[torch.Tensor] = None, y: Optional[torch.Tensor] = None,
                  dup_off: int = 0) -> torch.Tensor:
    """3x3 conv from x fp32 NCHW (<= 4 channels) to NHWC fp16; weight [Cout][9 Cin] tap-major.  y: a caller's buffer (with dup_off)."""
    n, cin, h, w = x.shape
    cout = weight.shape[0]
    if y is None:
        y = torch.empty(n, h, w, cout, dtype=torch.float16, device=x.device)
    check(lib().ld_op_small_conv_in(_p(x), _p(scale_sigma), _p(pre_w), _p(pre_b), _p(weight), _p(bias), _p(y), n, cin, h, w, cout, dup_off,
                                    _stream()), "ld_op_small_conv_in")
    return y


def small_conv_out(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, mode: int, x_in: Optional[torch.Tensor] = None,
                   sigma: Optional[torch.Tensor] = None, in_mod: int = 0) -> torch.Tensor:
    """3x3 conv from x fp16 NHWC to <= 4 channels, fp32; weight [Cout][9 Cin].  mode 0: x_in - fp16(v) sigma (NCHW), 1: clamp((v + 1) / 2)
    (NHWC), 2: v (NCHW)."""
    n, h, w, cin = x.shape
    cout = weight.shape[0]
    out = torch.empty((n, h, w, cout) if mode == 1 else (n, cout, h, w), dtype=torch.float32, device=x.device)
    check(lib().ld_op_small_conv_out(_p(x), _p(weight), _p(bias), n, h, w, cin, cout, mode, _p(x_in), _p(sigma), in_mod, _p(out), _stream()),
          "ld_op_small_conv_out")
    return out


def small_pointwise(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    n, hw, c = x.shape
    out = torch.empty(n, c, hw, dtype=torch.float32, device=x.device)
    check(lib().ld_op_small_pointwise(_p(x), _p(weight), _p(bias), _p(out), n, hw, c, _stream()), "ld_op_small_pointwise")
    return out


def vae_out_finish(t8: torch.Tensor, cout: int) -> torch.Tensor:
    npix = t8.numel() // 8
    out = torch.empty(npix, cout, dtype=torch.float32, device=t8.device)
    check(lib().ld_op_vae_out_finish(_p(t8), _p(out), npix, cout, _stream()), "ld_op_vae_out_finish")
    return out


def timestep_embed_mod(sigma: torch.Tensor, log_sigmas: torch.Tensor, dim: int, n: int, sigma_mod: int):
    out = torch.empty(n, dim, dtype=torch.float16, device=sigma.device)
    t = torch.empty(n, dtype=torch.float32, device=sigma.device)
    check(lib().ld_op_timestep_embed_mod(_p(sigma), _p(log_sigmas), log_sigmas.numel(), n, dim, _p(out), _p(t), sigma_mod, _stream()),
          "ld_op_timestep_embed_mod")
    return out, t


def ctx_pad(src: torch.Tensor, tp: int) -> torch.Tensor:
    n, t, d = src.shape
    dst = torch.empty(n, tp, d, dtype=torch.float16, device=src.device)
    check(lib().ld_op_ctx_pad(_p(src), F32 if src.dtype == torch.float32 else F16, n, t, tp, d, _p(dst), _stream()), "ld_op_ctx_pad")
    return dst


def context_kv(ctx16: torch.Tensor, wk: torch.Tensor, wv: torch.Tensor):
    """The cross-attention operands the UNet projects once per context: ctx16 [n, tp, d] (ctx_pad), wk / wv [c, d] ->
    (k [n, tp, c], vt [n, c, tp]) by the launches of ld_unet_set_context."""
    n, tp, d = ctx16.shape
    c = wk.shape[0]
    k = torch.empty(n, tp, c, dtype=torch.float16, device=ctx16.device)
    vt = torch.empty(n, c, tp, dtype=torch.float16, device=ctx16.device)
    check(lib().ld_op_ctx_kv(_p(ctx16), _p(wk), _p(wv), n, tp, d, c, _p(k), _p(vt), _stream()), "ld_op_ctx_kv")
    return k, vt


def dup_halves_(*tensors: torch.Tensor) -> None:
    """Up to three contiguous tensors whose dim 0 is even: the first half of each is copied onto its second half, in one launch (the CFG pair's
    hand-over in front of the first cross-attention)."""
    assert 1 <= len(tensors) <= 3
    args = []
    for t in tensors:
        assert t.is_cuda and t.is_contiguous() and t.shape[0] % 2 == 0
        args += [t.data_ptr(), t.numel() * t.element_size() // 2]
    args += [None, 0] * (3 - len(tensors))
    check(lib().ld_op_dup_halves(*args, len(tensors), _stream()), "ld_op_dup_halves")


def mlp_out_fold(wpo: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor, bpo: torch.Tensor):
    c = wpo.shape[0]
    w_out = torch.empty(c, 5 * c, dtype=torch.float16, device=wpo.device)
    b_out = torch.empty(c, dtype=torch.float16, device=wpo.device)
    check(lib().ld_op_mlp_out_fold(_p(wpo), _p(w2), _p(b2), _p(bpo), c, _p(w_out), _p(b_out), _stream()), "ld_op_mlp_out_fold")
    return w_out, b_out


def ln_fold(weight: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, bias: Optional[torch.Tensor] = None):
    n, k = weight.shape
    w_out = torch.empty_like(weight)
    b_out = torch.empty(n, dtype=torch.float16, device=weight.device)
    wsum = torch.empty(n, dtype=torch.float32, device=weight.device)
    check(lib().ld_op_ln_fold(_p(weight), n, k, _p(gamma), _p(beta), _p(bias), _p(w_out), _p(b_out), _p(wsum), _stream()), "ld_op_ln_fold")
    return w_out, b_out, wsum


def cfg_combine(den2: torch.Tensor, cfg: float) -> torch.Tensor:
    """den2 = [uncond ; cond] stacked on dim 0 (fp32) -> uncond + (cond - uncond) * cfg   (cfg_function, LD.py:2594-2606)."""
    half = den2.shape[0] // 2
    out = torch.empty_like(den2[:half])
    check(lib().ld_op_cfg_combine(_p(den2), _p(out), float(cfg), out.numel(), _stream()), "ld_op_cfg_combine")
    return out


def axpby_(x: torch.Tensor, a: float, y: Optional[torch.Tensor] = None, b: float = 0.0, z: Optional[torch.Tensor] = None,
           c: float = 0.0) -> torch.Tensor:
    """x <- a*x + b*y + c*z in place on fp32 latents (the samplers' update arithmetic)."""
    check(lib().ld_op_axpby(_p(x), float(a), _p(y), float(b), _p(z), float(c), x.numel(), _stream()), "ld_op_axpby")
    return x


def bislerp(samples: torch.Tensor, width: int, height: int, tmp: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bislerp(samples, width, height) of LD.py:429-518 on the device: [n,c,h,w] -> [n,c,height,width] (fp32 math).  tmp: an fp32 [n,c,h,width]
    tensor that receives the width pass's result (the height pass's input), for a caller that wants to look at it."""
    x = samples.float().contiguous()
    n, c, h, w = x.shape
    if tmp is None:
        tmp = torch.empty(n, c, h, width, dtype=torch.float32, device=x.device)
    assert tmp.dtype == torch.float32 and tuple(tmp.shape) == (n, c, h, width)
    y = torch.empty(n, c, height, width, dtype=torch.float32, device=x.device)
    check(lib().ld_op_bislerp(_p(x), _p(tmp), _p(y), n, c, h, w, height, width, _stream()), "ld_op_bislerp")
    return y.to(samples.dtype)


# ------------------------------------------------------------------ the end convolutions of the upscaler and the preview decoder, for parity tests
# Weights fp16 [cout][9 cin], tap-major and channel-minor (what repack_conv_weight writes); x and the results NHWC.
def esrgan_first(x: torch.Tensor, wt: torch.Tensor, bias: torch.Tensor, y: torch.Tensor, y2: Optional[torch.Tensor] = None) -> torch.Tensor:
    """conv_first of RRDBNet: x fp32 [n,h,w,3] -> channels [0, 64) of y fp16 [n,h,w,ldy] (the rest of y untouched), and y2 [n,h,w,ldy2] likewise."""
    n, h, w, _ = x.shape
    check(lib().ld_op_esrgan_first(_p(x), _p(wt), _p(bias), _p(y), y.shape[-1], _p(y2), 0 if y2 is None else y2.shape[-1], n, h, w, _stream()),
          "ld_op_esrgan_first")
    return y


def esrgan_last(x: torch.Tensor, wt: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """conv_last of RRDBNet: the first 64 channels of x fp16 [n,h,w,ldx] -> fp32 [n,h,w,3]."""
    n, h, w, ldx = x.shape
    out = torch.empty(n, h, w, 3, dtype=torch.float32, device=x.device)
    check(lib().ld_op_esrgan_last(_p(x), ldx, _p(wt), _p(bias), _p(out), n, h, w, _stream()), "ld_op_esrgan_last")
    return out


def taesd_first(x: torch.Tensor, wt: torch.Tensor, bias: torch.Tensor, y: Optional[torch.Tensor] = None) -> torch.Tensor:
    """TAESD's clamp + first convolution + ReLU: latent fp32 [n,h,w,4] -> fp16 [n,h,w,64] (a new tensor, or the caller's y)."""
    n, h, w, _ = x.shape
    if y is None:
        y = torch.empty(n, h, w, 64, dtype=torch.float16, device=x.device)
    assert y.dtype == torch.float16 and tuple(y.shape) == (n, h, w, 64)
    check(lib().ld_op_taesd_first(_p(x), _p(wt), _p(bias), _p(y), n, h, w, _stream()), "ld_op_taesd_first")
    return y


def taesd_last(x: torch.Tensor, wt: torch.Tensor, bias: torch.Tensor, image: bool = True):
    """TAESD's last convolution and output map: x fp16 [n,h,w,64] -> (fp32 [n,h,w,3] in [-1, 1] nominally, uint8 [n,h,w,3] or None)."""
    n, h, w, _ = x.shape
    out = torch.empty(n, h, w, 3, dtype=torch.float32, device=x.device)
    img = torch.empty(n, h, w, 3, dtype=torch.uint8, device=x.device) if image else None
    check(lib().ld_op_taesd_last(_p(x), _p(wt), _p(bias), _p(out), _p(img), n, h, w, _stream()), "ld_op_taesd_last")
    return out, img


# ------------------------------------------------------------------ the halo-tile 64-channel convolutions of the upscaler and the preview decoder
# One call = one launch of the executors (esrgan.hip esrgan_run, taesd.hip taesd_run), on caller-owned NHWC fp16 buffers that the call writes
# in place where the executor does: the dense block's append into its own input buffer, the second store over a residual.
def esrgan_conv(x: torch.Tensor, cin: int, wt: torch.Tensor, bias: Optional[torch.Tensor], y: torch.Tensor, c_off: int, cout: int,
                slope: float = 0.0, r1: Optional[torch.Tensor] = None, s1: float = 1.0, r2: Optional[torch.Tensor] = None, s2: float = 1.0,
                y2: Optional[torch.Tensor] = None, up: bool = False) -> torch.Tensor:
    """One conv_block of RRDBNet: channels [0, cin) of x [n,hs,ws,ldx] -> channels [c_off, c_off + cout) of y [n,h,w,ldy] (y may be x itself when
    c_off >= cin), v = lrelu(conv + bias, slope) (slope 0: none), then s1 v + r1, then s2 v + r2 (the first cout channels of r1 / r2), and the
    same values into channels [0, cout) of y2 (which may be r2).  up: x is [n,h/2,w/2,ldx], read through a nearest-2x upsampling."""
    n, h, w, ldy = y.shape
    ld = lambda t: 0 if t is None else t.shape[-1]
    check(lib().ld_op_esrgan_conv_y2(_p(x), x.shape[-1], cin, n, h, w, int(up), _p(wt), _p(bias), _p(y), ldy, c_off, cout, slope, _p(r1), ld(r1), s1,
                                     _p(r2), ld(r2), s2, _p(y2), ld(y2), _stream()), "ld_op_esrgan_conv_y2")
    return y


def taesd_conv(x: torch.Tensor, wt: torch.Tensor, bias: Optional[torch.Tensor], y: torch.Tensor, residual: Optional[torch.Tensor] = None,
               relu: bool = False, up: bool = False) -> torch.Tensor:
    """One convolution of a TAESD Block, or the one behind an nn.Upsample: x [n,hs,ws,64] -> y [n,h,w,64] = relu?(conv + bias? + residual?), written
    into the caller's y (the executor's rotating buffers); up: x is [n,h/2,w/2,64], read through a nearest-2x upsampling."""
    n, h, w, _ = y.shape
    check(lib().ld_op_taesd_conv(_p(x), n, h, w, int(up), _p(wt), _p(bias), _p(residual), int(relu), _p(y), _stream()), "ld_op_taesd_conv")
    return y


# ------------------------------------------------------------------ 8-bit image ops (image.hip): UltimateSDUpscale's tile plumbing
# uint8 images [H, W, C] (masks [H, W]) on the device; a view whose pixels are contiguous within a row (a crop) is taken as pointer + pitch.
# Integer arithmetic, bit-identical to Pillow.  These five — u8_from_f32, f32_from_u8, u8_resample, u8_region_mask, u8_composite_ — are the
# seam usdu.py works through.
_RESAMPLE_FILTERS = {"lanczos": 3.0, "bicubic": 2.0}


def _filter_value(filt: str, x: float) -> float:
    if filt == "lanczos":          # sinc(x) sinc(x / 3) on [-3, 3)
        if not -3.0 <= x < 3.0:
            return 0.0
        sinc = lambda v: 1.0 if v == 0.0 else math.sin(math.pi * v) / (math.pi * v)
        return sinc(x) * sinc(x / 3.0)
    a, x = -0.5, abs(x)            # bicubic, a = -0.5
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


_COEF_ROWS = {}
_COEF_DEV = {}


def resample_coeffs(in_size: int, out_size: int, filt: str = "lanczos"):
    """One axis of Pillow's precompute_coeffs + normalize_coeffs_8bpc, in double on the host: (rows, k) with rows[out] = [first input
    sample, tap count, k taps in fixed point with 22 fractional bits].  Cached per (in, out, filter)."""
    key = (in_size, out_size, filt)
    if key not in _COEF_ROWS:
        support = _RESAMPLE_FILTERS[filt]
        scale = in_size / out_size
        fs = max(scale, 1.0)
        sup = support * fs
        k = int(math.ceil(sup)) * 2 + 1
        rows = []
        for xx in range(out_size):
            center = (xx + 0.5) * scale
            lo = max(int(center - sup + 0.5), 0)
            hi = min(int(center + sup + 0.5), in_size)
            w = [_filter_value(filt, (j + lo - center + 0.5) / fs) for j in range(hi - lo)]
            ww = sum(w)
            if ww != 0.0:
                w = [v / ww for v in w]
            kk = [int(0.5 + v * (1 << 22)) if v >= 0 else int(-0.5 + v * (1 << 22)) for v in w]
            # the kernels accumulate in int32: 2^21 + 255 sum |tap| must stay below 2^31 (sum |k| < 2; Lanczos is about 1.4)
            assert (1 << 21) + 255 * sum(abs(v) for v in kk) < (1 << 31), "resample taps overflow the int32 accumulator"
            rows.append([lo, hi - lo] + kk + [0] * (k - len(kk)))
        _COEF_ROWS[key] = (rows, k)
    return _COEF_ROWS[key]


def _coeffs_on(device, in_size: int, out_size: int, filt: str):
    d = torch.device(device)
    key = (in_size, out_size, filt, d.index if d.index is not None else torch.cuda.current_device())
    if key not in _COEF_DEV:                      # uploaded once
        rows, k = resample_coeffs(in_size, out_size, filt)
        _COEF_DEV[key] = (torch.tensor(rows, dtype=torch.int32).to(d), k)
    return _COEF_DEV[key]


def _u8_image(t: torch.Tensor):
    """(pointer, row pitch in bytes, h, w, c) of a uint8 image view [H, W] or [H, W, C] whose rows are dense."""
    assert t.is_cuda and t.dtype == torch.uint8 and t.dim() in (2, 3), "a uint8 device image [H, W] or [H, W, C]"
    c = 1 if t.dim() == 2 else t.shape[2]
    dense = t.stride(1) == 1 if t.dim() == 2 else (t.stride(2) == 1 and t.stride(1) == c)
    assert dense and t.stride(0) >= t.shape[1] * c, "pixels must be contiguous within a row"
    return t.data_ptr(), t.stride(0), t.shape[0], t.shape[1], c


def u8_from_f32(x: torch.Tensor) -> torch.Tensor:
    """tensor_to_pil (LD.py:7445-7449) without the PIL object: uint8(clip(255 x, 0, 255)), a truncation in fp32."""
    x = x.contiguous()
    assert x.is_cuda and x.dtype == torch.float32
    y = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    check(lib().ld_op_u8_from_f32(x.data_ptr(), y.data_ptr(), x.numel(), _stream()), "ld_op_u8_from_f32")
    return y


def f32_from_u8(x: torch.Tensor) -> torch.Tensor:
    """pil_to_tensor (LD.py:7452-7456): x / 255 as a correctly rounded fp32 division."""
    x = x.contiguous()
    assert x.is_cuda and x.dtype == torch.uint8
    y = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    check(lib().ld_op_f32_from_u8(x.data_ptr(), y.data_ptr(), x.numel(), _stream()), "ld_op_f32_from_u8")
    return y


def u8_resample(src: torch.Tensor, size, filt: str = "lanczos") -> torch.Tensor:
    """Image.resize(size = (w, h), LANCZOS / BICUBIC) of a uint8 image or of a crop of one (a view): horizontal pass, then vertical, each
    skipped when its size does not change (both: a copy)."""
    ptr, pitch, h, w, c = _u8_image(src)
    ow, oh = int(size[0]), int(size[1])
    dst = torch.empty((oh, ow) + tuple(src.shape[2:]), dtype=torch.uint8, device=src.device)
    hco, hk = _coeffs_on(src.device, w, ow, filt) if ow != w else (None, 0)
    vco, vk = _coeffs_on(src.device, h, oh, filt) if oh != h else (None, 0)
    tmp = torch.empty(lib().ld_op_u8_resample_tmp_bytes(h, ow, c), dtype=torch.uint8, device=src.device) if hco is not None and vco is not None else None
    check(lib().ld_op_u8_resample(ptr, pitch, w, h, c, dst.data_ptr(), ow * c, ow, oh, _p(hco), hk, _p(vco), vk, _p(tmp), _stream()), "ld_op_u8_resample")
    return dst


def u8_box_weights(radius: float):
    """(R, ww, fw) of one box pass of GaussianBlur(radius): the integer radius and the two fixed-point weights."""
    import ctypes
    r, ww, fw = ctypes.c_int(0), ctypes.c_uint(0), ctypes.c_uint(0)
    check(lib().ld_op_u8_box_weights(float(radius), ctypes.byref(r), ctypes.byref(ww), ctypes.byref(fw)), "ld_op_u8_box_weights")
    return r.value, ww.value, fw.value


def u8_blur_reach(radius: float) -> int:
    """How far GaussianBlur(radius) reads along one axis: three passes of R + 1 samples."""
    return 3 * (u8_box_weights(radius)[0] + 1)


def _blur_window(hw, region, radius: float):
    """The region (x1, y1, x2, y2) grown by the blur's reach and clipped to the image: a blur of that window, replicating at ITS border,
    equals the blur of the whole image on the region (a window side is either the image's or out of the region's reach)."""
    reach = u8_blur_reach(radius)
    x1, y1, x2, y2 = region
    return max(x1 - reach, 0), max(y1 - reach, 0), min(x2 + reach, hw[1]), min(y2 + reach, hw[0])


def u8_gaussian_blur(mask: torch.Tensor, radius: float, region=None) -> torch.Tensor:
    """ImageFilter.GaussianBlur(radius) of a one-channel uint8 image [H, W].  region (x1, y1, x2, y2): only that part of the result is
    wanted — the window around it is blurred and the region returned (a view), equal to the same part of the full-image blur."""
    wx1, wy1, wx2, wy2 = (0, 0, mask.shape[1], mask.shape[0]) if region is None else _blur_window(mask.shape, region, radius)
    win = mask[wy1:wy2, wx1:wx2]
    ptr, pitch, h, w, _ = _u8_image(win)
    dst = torch.empty(h, w, dtype=torch.uint8, device=mask.device)
    tmp = torch.empty(lib().ld_op_u8_blur_tmp_bytes(w, h), dtype=torch.uint8, device=mask.device)
    check(lib().ld_op_u8_gaussian_blur(ptr, pitch, dst.data_ptr(), w, w, h, float(radius), tmp.data_ptr(), _stream()), "ld_op_u8_gaussian_blur")
    if region is None:
        return dst
    return dst[region[1] - wy1:region[3] - wy1, region[0] - wx1:region[2] - wx1]


def u8_mask(h: int, w: int, rect, pattern: Optional[torch.Tensor] = None, device=None) -> torch.Tensor:
    """A [h, w] mask: 0 except the rectangle rect = (x, y, width, height), which may hang over any edge: 255, or `pattern` [height, width]."""
    device = pattern.device if pattern is not None else device
    dst = torch.empty(h, w, dtype=torch.uint8, device=device)
    pp, ppitch = (None, 0) if pattern is None else (_u8_image(pattern)[0], pattern.stride(0))
    with torch.cuda.device(dst.device):
        check(lib().ld_op_u8_mask(dst.data_ptr(), w, w, h, int(rect[0]), int(rect[1]), int(rect[2]), int(rect[3]), pp, ppitch, _stream()), "ld_op_u8_mask")
    return dst


def u8_region_mask(hw, rect, pattern: Optional[torch.Tensor], radius: float, region, device) -> torch.Tensor:
    """One job's alpha: the mask of a canvas of size hw = (H, W) that is 0 except `rect` (see u8_mask), blurred with GaussianBlur(radius)
    when radius > 0, on the crop region (x1, y1, x2, y2) only.  Nothing of canvas size is built: the mask is written into the window the
    blur needs (see u8_gaussian_blur) and blurred there."""
    wx1, wy1, wx2, wy2 = _blur_window(hw, region, radius) if radius > 0 else region
    win = u8_mask(wy2 - wy1, wx2 - wx1, (rect[0] - wx1, rect[1] - wy1, rect[2], rect[3]), pattern, device)
    if not radius > 0:
        return win
    return u8_gaussian_blur(win, radius, (region[0] - wx1, region[1] - wy1, region[2] - wx1, region[3] - wy1))


def u8_composite_(canvas: torch.Tensor, tile: torch.Tensor, alpha: torch.Tensor, x0: int, y0: int) -> torch.Tensor:
    """canvas[y0:y0+h, x0:x0+w] = div255(tile a + canvas (255 - a)) in place — process_images' paste / putalpha / alpha_composite /
    convert("RGB") chain (LD.py:7718-7736) over an opaque canvas.  The rest of the canvas is untouched."""
    cp, cpitch, ch, cw, c = _u8_image(canvas)
    tp, tpitch, h, w, tc = _u8_image(tile)
    ap, apitch, ah, aw, _ = _u8_image(alpha)
    assert tc == c and (ah, aw) == (h, w), "tile and alpha must have the region's size"
    check(lib().ld_op_u8_composite(cp, cpitch, cw, ch, tp, tpitch, ap, apitch, int(x0), int(y0), w, h, c, _stream()), "ld_op_u8_composite")
    return canvas


# ------------------------------------------------------------------ fp32 image ops (detail/detail_image.hip): the Detailer's per-segment plumbing
# The canvas is fp32 [H, W, C] on the device, a mask fp32 [H, W]; a view whose pixels are contiguous within a row is taken as pointer + pitch (in
# floats).  With u8_resample, u8_from_f32 and f32_from_u8 above these three are the seam detailer.py works through.  A bad argument is a
# ValueError on the host, before anything is launched.
def _image_view(t: torch.Tensor, dtype, dims, what: str):
    """(pointer, row pitch in elements, h, w, c) of a device image view [H, W] or [H, W, C] of `dtype` whose rows are dense."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{what}: a tensor on the device is needed, got {getattr(t, 'device', type(t).__name__)}")
    if t.dtype != dtype:
        raise ValueError(f"{what}: dtype {t.dtype}, expected {dtype}")
    if t.dim() != dims or min(t.shape) < 1:
        raise ValueError(f"{what}: shape {tuple(t.shape)}, expected {'[H, W]' if dims == 2 else '[H, W, C]'} with no empty side")
    c = 1 if dims == 2 else t.shape[2]
    dense = t.stride(1) == 1 if dims == 2 else (t.stride(2) == 1 and t.stride(1) == c)
    if not 1 <= c <= 4 or not dense or (t.shape[0] > 1 and t.stride(0) < t.shape[1] * c):
        raise ValueError(f"{what}: 1 to 4 channels, pixels contiguous within a row (shape {tuple(t.shape)}, strides {t.stride()})")
    return t.data_ptr(), max(t.stride(0), t.shape[1] * c), t.shape[0], t.shape[1], c


def u8_crop_from_f32(canvas: torch.Tensor, x1: int, y1: int, x2: int, y2: int) -> torch.Tensor:
    """tensor2pil (LD.py:8505-8509) of canvas[y1:y2, x1:x2] without the PIL object: uint8(clip(255 x, 0, 255)), a truncation in fp32, as a dense
    uint8 [y2 - y1, x2 - x1, C].  The canvas is not written."""
    ptr, pitch, ch, cw, c = _image_view(canvas, torch.float32, 3, "canvas")
    x1, y1, x2, y2 = int(x1), int(y1), int(x2), int(y2)
    if not (0 <= x1 < x2 <= cw and 0 <= y1 < y2 <= ch):
        raise ValueError(f"the window [{x1}, {y1}, {x2}, {y2}] does not lie inside the {cw} x {ch} canvas")
    dst = torch.empty(y2 - y1, x2 - x1, c, dtype=torch.uint8, device=canvas.device)
    with torch.cuda.device(canvas.device):
        check(lib().ld_op_f32_crop_u8(ptr, pitch, cw, ch, c, x1, y1, x2, y2, dst.data_ptr(), (x2 - x1) * c, _stream()), "ld_op_f32_crop_u8")
    return dst


_GAUSS_TAPS = {}


def gaussian_taps(feather: int, sigma: float = 10.0) -> torch.Tensor:
    """torchvision's _get_gaussian_kernel1d(2 feather + 1, sigma) as it computes it, in torch fp32 on the host: [2 feather + 1]."""
    x = torch.linspace(-float(feather), float(feather), steps=2 * feather + 1, dtype=torch.float32)
    pdf = torch.exp(-0.5 * (x / sigma).pow(2))
    return pdf / pdf.sum()


def _taps_on(device, feather: int, sigma: float) -> torch.Tensor:
    d = torch.device(device)
    key = (feather, float(sigma), d.index if d.index is not None else torch.cuda.current_device())
    if key not in _GAUSS_TAPS:                    # uploaded once
        _GAUSS_TAPS[key] = gaussian_taps(feather, float(sigma)).to(d)
    return _GAUSS_TAPS[key]


def f32_blur_max_feather() -> int:
    """The largest feather f32_gaussian_blur takes: its 2 feather + 1 taps are staged in LDS."""
    return lib().ld_op_f32_blur_max_feather()


def f32_gaussian_blur(mask: torch.Tensor, feather: int, sigma: float = 10.0) -> torch.Tensor:
    """tensor_gaussian_blur_mask (LD.py:8979-9004): torchvision's GaussianBlur(2 feather + 1, sigma) of an fp32 mask [H, W] (or a window of one: a
    view) with reflect padding -> a new dense fp32 [H, W].  Taps in torch fp32 as torchvision builds them, two passes, every product and sum
    rounded to fp32 in ascending tap order.  feather 0: a copy."""
    ptr, pitch, h, w, _ = _image_view(mask, torch.float32, 2, "mask")
    feather = int(feather)
    if feather < 0 or feather >= min(h, w):
        raise ValueError(f"feather={feather} must be at least 0 and smaller than both sides of the {w} x {h} mask (the blur pads by reflection)")
    if feather > f32_blur_max_feather():
        raise ValueError(f"feather={feather} is above the kernel's limit of {f32_blur_max_feather()} (its taps are staged in LDS)")
    if not float(sigma) > 0.0:
        raise ValueError(f"sigma={sigma} must be positive")
    dst = torch.empty(h, w, dtype=torch.float32, device=mask.device)
    taps = tmp = None
    if feather > 0:
        taps = _taps_on(mask.device, feather, sigma)
        tmp = torch.empty(lib().ld_op_f32_blur_tmp_bytes(w, h), dtype=torch.uint8, device=mask.device)
    with torch.cuda.device(mask.device):
        check(lib().ld_op_f32_gaussian_blur(ptr, pitch, dst.data_ptr(), w, w, h, feather, _p(taps), _p(tmp), _stream()), "ld_op_f32_gaussian_blur")
    return dst


def f32_paste_u8_(canvas: torch.Tensor, tile: torch.Tensor, alpha: torch.Tensor, x0: int, y0: int) -> torch.Tensor:
    """pil2tensor + tensor_paste (LD.py:8888-8889, 9355-9373) in place: canvas[y0:y0+h, x0:x0+w] = (1 - a) canvas + a (tile / 255) on the uint8 tile's window
    clipped to the canvas, every fp32 operation rounded on its own.  The rest of the canvas is untouched.  -> canvas"""
    cp, cpitch, ch, cw, c = _image_view(canvas, torch.float32, 3, "canvas")
    tp, tpitch, th, tw, tc = _image_view(tile, torch.uint8, 3, "tile")
    ap, apitch, ah, aw, _ = _image_view(alpha, torch.float32, 2, "alpha")
    if tile.device != canvas.device or alpha.device != canvas.device:
        raise ValueError(f"canvas, tile and alpha must be on one device, got {canvas.device}, {tile.device}, {alpha.device}")
    if tc != c:
        raise ValueError(f"a tile of {tc} channels for a canvas of {c}")
    if (ah, aw) != (th, tw):
        raise ValueError(f"alpha of shape {(ah, aw)} for a tile of {(th, tw)}")
    x0, y0 = int(x0), int(y0)
    if not (0 <= x0 < cw and 0 <= y0 < ch):
        raise ValueError(f"the tile's origin ({x0}, {y0}) does not lie inside the {cw} x {ch} canvas")
    with torch.cuda.device(canvas.device):
        check(lib().ld_op_f32_paste_u8(cp, cpitch, cw, ch, c, tp, tpitch, ap, apitch, tw, th, x0, y0, _stream()), "ld_op_f32_paste_u8")
    return canvas


# ------------------------------------------------------------------ the masked sampler step (inpaint/inpaint.hip)
# The two blends sampling.KSamplerX0Inpaint makes around the model call, on contiguous fp32 latents [B, C, h, w]; the mask is [Bm, Cm, h, w] with
# Bm in {1, B} and Cm in {1, C} and is broadcast in the kernel.  Every fp32 operation is rounded on its own, in the order of the expression.  A
# bad argument is a ValueError on the host, before anything is launched.  For tensors on the host (the sampler's CPU tests run its loops on a
# toy denoiser there) the same expression is evaluated with torch operations in the same order; a device tensor never takes that path.
def _inpaint_args(what: str, x: torch.Tensor, mask: torch.Tensor, others: dict):
    """-> (B, C, HW, Bm, Cm) after the shape / dtype / device checks of both blends."""
    if not isinstance(x, torch.Tensor) or x.dim() != 4 or min(x.shape) < 1:
        raise ValueError(f"{what}: a latent [B, C, h, w] with no empty side is needed, got {tuple(getattr(x, 'shape', ()))}")
    b, c, h, w = x.shape
    if x.numel() >= 1 << 31:
        raise ValueError(f"{what}: a latent of {x.numel()} elements: the kernels index in 32 bits, fewer than 2^31 are needed")
    if not isinstance(mask, torch.Tensor) or mask.dim() != 4 or tuple(mask.shape[2:]) != (h, w) or mask.shape[0] not in (1, b) or mask.shape[1] not in (1, c):
        raise ValueError(f"{what}: mask of shape {tuple(getattr(mask, 'shape', ()))} for a latent of {tuple(x.shape)}: expected [1 or {b}, 1 or {c}, {h}, {w}]")
    for name, t in others.items():
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(x.shape):
            raise ValueError(f"{what}: {name} of shape {tuple(getattr(t, 'shape', ()))}, expected the latent's {tuple(x.shape)}")
    for name, t in dict(others, latent=x, mask=mask).items():
        if t.dtype != torch.float32:
            raise ValueError(f"{what}: {name} has dtype {t.dtype}, expected torch.float32")
        if t.device != x.device:
            raise ValueError(f"{what}: {name} is on {t.device}, the latent on {x.device}: one device is needed")
        if not t.is_contiguous():
            raise ValueError(f"{what}: {name} is not contiguous (shape {tuple(t.shape)}, strides {t.stride()})")
    return b, c, h * w, mask.shape[0], mask.shape[1]


def inpaint_in(x: torch.Tensor, mask: torch.Tensor, latent: torch.Tensor, noise: torch.Tensor, sigma: torch.Tensor,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = x * m + (noise * sigma[b] + latent) * (1 - m): what the model sees of a masked step — x where the mask is 1, the latent noised to this
    step's sigma (EPS.noise_scaling, max_denoise = False, LD.py:1267-1274) where it is 0.  sigma: fp32 [B] on x's device, read there.  `out`: where
    the result goes (a new tensor by default); it may be x."""
    others = {"latent_image": latent, "noise": noise}
    if out is not None:
        others["out"] = out
    b, c, hw, bm, cm = _inpaint_args("inpaint_in", x, mask, others)
    if not isinstance(sigma, torch.Tensor) or sigma.dtype != torch.float32 or tuple(sigma.shape) != (b,) or sigma.device != x.device or not sigma.is_contiguous():
        raise ValueError(f"inpaint_in: sigma must be a contiguous fp32 [{b}] on {x.device}, one value per sample, got "
                         f"{tuple(getattr(sigma, 'shape', ()))} {getattr(sigma, 'dtype', type(sigma).__name__)} on {getattr(sigma, 'device', None)}")
    if out is None:
        out = torch.empty_like(x)
    if not x.is_cuda:
        return out.copy_(x * mask + (noise * sigma.view(b, 1, 1, 1) + latent) * (1.0 - mask))
    with torch.cuda.device(x.device):
        check(lib().ld_op_inpaint_in(x.data_ptr(), mask.data_ptr(), latent.data_ptr(), noise.data_ptr(), sigma.data_ptr(), out.data_ptr(), b, c, hw, bm, cm,
                                     _stream()), "ld_op_inpaint_in")
    return out


def inpaint_out_(den: torch.Tensor, mask: torch.Tensor, latent: torch.Tensor) -> torch.Tensor:
    """den = den * m + latent * (1 - m) in place: the model's answer where the mask is 1, the latent itself where it is 0.  -> den"""
    b, c, hw, bm, cm = _inpaint_args("inpaint_out_", den, mask, {"latent_image": latent})
    if not den.is_cuda:
        return den.copy_(den * mask + latent * (1.0 - mask))
    with torch.cuda.device(den.device):
        check(lib().ld_op_inpaint_out(den.data_ptr(), mask.data_ptr(), latent.data_ptr(), b, c, hw, bm, cm, _stream()), "ld_op_inpaint_out")
    return den


# ------------------------------------------------------------------ regional conditioning (regional/regional.hip)
# The two launches sampling.sampling_function makes around the model calls of a step whose conditioning entries carry an area, a mask or a
# strength, on contiguous fp32 latents [B, C, H, W]: `regional_gather` builds the model input of one group of entries (windows of one h x w),
# `regional_combine` reduces every group's output to the guided result.  Every fp32 operation is rounded on its own, in the order of the
# expression (ld_mi355x.h).  A bad argument is a ValueError on the host, before anything is launched.  For tensors on the host the same
# expression is evaluated with torch operations in the same order; a device tensor never takes that path.
REGIONAL_MAX_ENTRIES = 16


class RegionalEntry(NamedTuple):
    """One conditioning entry of a step, as regional_combine reads it: its `list` (0: cond, 1: uncond), where its output lies (rows
    [slot * B, (slot + 1) * B) of outs[group]), its area (h, w, y0, x0) on the latent, its strength, and its mask ([Bm, H, W] on the latent's
    grid, Bm in {1, B}, or None) with the mask's strength."""
    list: int
    group: int
    slot: int
    area: tuple
    strength: float = 1.0
    mask: Optional[torch.Tensor] = None
    mask_strength: float = 1.0


def _regional_latent(what: str, x, name: str = "the latent"):
    if not isinstance(x, torch.Tensor) or x.dim() != 4 or min(x.shape) < 1:
        raise ValueError(f"{what}: {name} must be [B, C, H, W] with no empty side, got {tuple(getattr(x, 'shape', ()))}")
    if x.dtype != torch.float32:
        raise ValueError(f"{what}: {name} has dtype {x.dtype}, expected torch.float32")
    if not x.is_contiguous():
        raise ValueError(f"{what}: {name} is not contiguous (shape {tuple(x.shape)}, strides {x.stride()})")
    if x.numel() >= 1 << 31:
        raise ValueError(f"{what}: {name} has {x.numel()} elements: the kernels index in 32 bits, fewer than 2^31 are needed")


def _regional_area(what: str, area, H: int, W: int):
    if len(area) != 4 or not all(isinstance(v, int) and not isinstance(v, bool) for v in area):
        raise ValueError(f"{what}: an area is four ints (h, w, y0, x0), got {area!r}")
    h, w, y0, x0 = area
    if h < 1 or w < 1:
        raise ValueError(f"{what}: area {tuple(area)} has a side < 1")
    if y0 < 0 or x0 < 0 or y0 + h > H or x0 + w > W:
        raise ValueError(f"{what}: area {tuple(area)} leaves the {H} x {W} latent")
    return h, w, y0, x0


def regional_gather(x: torch.Tensor, windows, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[(j * B + b), c, y, x] = x[b, c, y0_j + y, x0_j + x]: the k windows (h, w, y0, x0) of one group, all of one h x w, as ONE batch
    [k * B, C, h, w] — the model input of the group (k windows that are the whole latent: the latent k times)."""
    what = "regional_gather"
    _regional_latent(what, x)
    b, c, H, W = x.shape
    windows = [tuple(v) for v in windows]
    if not 1 <= len(windows) <= REGIONAL_MAX_ENTRIES:
        raise ValueError(f"{what}: {len(windows)} windows; 1 to {REGIONAL_MAX_ENTRIES} are needed")
    areas = [_regional_area(what, v, H, W) for v in windows]
    h, w = areas[0][:2]
    if any(a[:2] != (h, w) for a in areas):
        raise ValueError(f"{what}: the windows of one group have one shape, got {sorted({a[:2] for a in areas})}")
    k = len(areas)
    if k * b * c * h * w >= 1 << 31:
        raise ValueError(f"{what}: a batch of {k * b * c * h * w} elements: the kernels index in 32 bits, fewer than 2^31 are needed")
    if out is None:
        out = torch.empty((k * b, c, h, w), dtype=torch.float32, device=x.device)
    else:
        _regional_latent(what, out, "out")
        if tuple(out.shape) != (k * b, c, h, w) or out.device != x.device:
            raise ValueError(f"{what}: out of shape {tuple(out.shape)} on {out.device}, expected {(k * b, c, h, w)} on {x.device}")
    if not x.is_cuda:
        return out.copy_(torch.cat([x[:, :, y0:y0 + h, x0:x0 + w] for _, _, y0, x0 in areas]))
    from ._lib import RegionalWindow
    tab = (RegionalWindow * k)(*[RegionalWindow(y0, x0) for _, _, y0, x0 in areas])
    with torch.cuda.device(x.device):
        check(lib().ld_op_regional_gather(x.data_ptr(), out.data_ptr(), b, c, H, W, h, w, tab, k, _stream()), "ld_op_regional_gather")
    return out


def _regional_ramp(h: int, from_end: bool) -> torch.Tensor:
    """the factors of one feathered edge along an axis of h pixels: 0.125 * (t + 1) for the pixel t < 8 from the edge, 1 beyond"""
    r = torch.ones(h)
    n = min(8, h)
    r[:n] = 0.125 * (torch.arange(n, dtype=torch.float32) + 1.0)
    return r.flip(0) if from_end else r


def regional_combine(outs, entries, cond_scale: float, shape, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The guided result [B, C, H, W] (`shape`) of one step: u + (c - u) * cond_scale, where each list's prediction is
    sum(out_e * mult_e) / (1e-37 + sum(mult_e)) over its entries e that cover the pixel, accumulated in the order of `entries`:
    mult = (mask ? mask[b % Bm] * mask_strength : 1) * strength, and without a mask the eight-pixel ramps 0.125 * (t + 1) at the area's top,
    bottom, left and right edges that are not edges of the latent, multiplied in in that order.  A pixel that no entry of a list covers gives 0
    for that list.  outs: the groups' model outputs [k_g * B, C, h_g, w_g]; entries: RegionalEntry rows."""
    what = "regional_combine"
    if len(shape) != 4 or min(shape) < 1:
        raise ValueError(f"{what}: shape must be (B, C, H, W) with no empty side, got {tuple(shape)}")
    b, c, H, W = (int(v) for v in shape)
    if b * c * H * W >= 1 << 31:
        raise ValueError(f"{what}: a latent of {b * c * H * W} elements: the kernels index in 32 bits, fewer than 2^31 are needed")
    outs, entries = list(outs), [RegionalEntry(*e) for e in entries]
    if not outs or not 1 <= len(entries) <= REGIONAL_MAX_ENTRIES:
        raise ValueError(f"{what}: {len(outs)} group outputs and {len(entries)} entries; at least one group and 1 to {REGIONAL_MAX_ENTRIES} entries are needed")
    for g, o in enumerate(outs):
        _regional_latent(what, o, f"outs[{g}]")
        if o.shape[0] % b or o.shape[1] != c or o.device != outs[0].device:
            raise ValueError(f"{what}: outs[{g}] of shape {tuple(o.shape)} on {o.device}: rows in multiples of {b}, {c} channels, on {outs[0].device}")
    dev = outs[0].device
    seen = set()
    for i, e in enumerate(entries):
        h, w, y0, x0 = _regional_area(f"{what}: entry {i}", e.area, H, W)
        if e.list not in (0, 1):
            raise ValueError(f"{what}: entry {i}: list {e.list!r}, expected 0 (cond) or 1 (uncond)")
        if not isinstance(e.group, int) or not 0 <= e.group < len(outs):
            raise ValueError(f"{what}: entry {i}: group {e.group!r} of {len(outs)}")
        o = outs[e.group]
        if tuple(o.shape[2:]) != (h, w) or not isinstance(e.slot, int) or not 0 <= e.slot < o.shape[0] // b or (e.group, e.slot) in seen:
            raise ValueError(f"{what}: entry {i}: area {tuple(e.area)}, slot {e.slot!r} do not fit outs[{e.group}] of shape {tuple(o.shape)} (or the slot is taken)")
        seen.add((e.group, e.slot))
        if e.mask is not None:
            m = e.mask
            if not isinstance(m, torch.Tensor) or m.dim() != 3 or tuple(m.shape[1:]) != (H, W) or m.shape[0] not in (1, b):
                raise ValueError(f"{what}: entry {i}: mask of shape {tuple(getattr(m, 'shape', ()))}, expected [1 or {b}, {H}, {W}]")
            if m.dtype != torch.float32 or m.device != dev or not m.is_contiguous():
                raise ValueError(f"{what}: entry {i}: the mask must be contiguous fp32 on {dev}, got {m.dtype} on {m.device}, strides {m.stride()}")
    if out is None:
        out = torch.empty((b, c, H, W), dtype=torch.float32, device=dev)
    else:
        _regional_latent(what, out, "out")
        if tuple(out.shape) != (b, c, H, W) or out.device != dev:
            raise ValueError(f"{what}: out of shape {tuple(out.shape)} on {out.device}, expected {(b, c, H, W)} on {dev}")
    if not dev.type == "cuda":
        num = [torch.zeros((b, c, H, W)), torch.zeros((b, c, H, W))]
        den = [torch.full((b, c, H, W), 1e-37), torch.full((b, c, H, W), 1e-37)]
        for e in entries:
            h, w, y0, x0 = e.area
            o = outs[e.group][e.slot * b:(e.slot + 1) * b]
            if e.mask is not None:
                mult = ((e.mask[:, y0:y0 + h, x0:x0 + w] * e.mask_strength) * e.strength)[:, None]
            else:
                mult = torch.ones((1, 1, h, w)) * e.strength
                if y0 != 0:
                    mult = mult * _regional_ramp(h, False).view(1, 1, h, 1)
                if y0 + h < H:
                    mult = mult * _regional_ramp(h, True).view(1, 1, h, 1)
                if x0 != 0:
                    mult = mult * _regional_ramp(w, False).view(1, 1, 1, w)
                if x0 + w < W:
                    mult = mult * _regional_ramp(w, True).view(1, 1, 1, w)
            num[e.list][:, :, y0:y0 + h, x0:x0 + w] += o * mult
            den[e.list][:, :, y0:y0 + h, x0:x0 + w] += mult
        cond, uncond = num[0] / den[0], num[1] / den[1]
        return out.copy_(uncond + (cond - uncond) * cond_scale)
    from ._lib import RegionalEntry as _Entry
    tab = (_Entry * len(entries))()
    for t, e in zip(tab, entries):
        h, w, y0, x0 = e.area
        o = outs[e.group]
        t.out = o.data_ptr() + e.slot * b * c * h * w * 4
        t.mask = None if e.mask is None else e.mask.data_ptr()
        t.list, t.mask_batch = e.list, 1 if e.mask is None else e.mask.shape[0]
        t.y0, t.x0, t.h, t.w = y0, x0, h, w
        t.strength, t.mask_strength = e.strength, e.mask_strength
    with torch.cuda.device(dev):
        check(lib().ld_op_regional_combine(tab, len(entries), float(cond_scale), out.data_ptr(), b, c, H, W, _stream()), "ld_op_regional_combine")
    return out


# ------------------------------------------------------------------ ControlNet's kernels (control/control.hip)
def control_add_(ts, rs, strength: float, n: Optional[int] = None, r_n: Optional[int] = None):
    """In place, ONE launch over up to 16 (t, r) pairs: t = fp16(float(t) + strength * float(r)); t [n, ...] and r [r_n, ...] fp16 on one
    device, r_n dividing n: sample s reads residual sample s % r_n.  The bits of (t.float() + strength * r.float()).half()."""
    import ctypes as C
    if len(ts) != len(rs) or not 1 <= len(ts) <= CONTROL_MAX_SEGMENTS:
        raise LDError(ERR_SHAPE, f"control_add: {len(ts)} segments, {len(rs)} residuals (1 .. {CONTROL_MAX_SEGMENTS})")
    n = ts[0].shape[0] if n is None else n
    r_n = rs[0].shape[0] if r_n is None else r_n
    for t, r in zip(ts, rs):
        assert t.dtype == torch.float16 and r.dtype == torch.float16 and t.is_cuda and r.is_cuda
        if t.numel() % n or r.numel() * n != t.numel() * r_n:
            raise LDError(ERR_SHAPE, f"control_add: segment {tuple(t.shape)} against residual {tuple(r.shape)} with n = {n}, r_n = {r_n}")
    tp = (C.c_void_p * len(ts))(*[_p(t) for t in ts])
    rp = (C.c_void_p * len(ts))(*[_p(r) for r in rs])
    per = (C.c_longlong * len(ts))(*[t.numel() // n for t in ts])
    with torch.cuda.device(ts[0].device):
        check(lib().ld_op_control_add(tp, rp, per, len(ts), n, r_n, float(strength), _stream()), "ld_op_control_add")
    return ts


def hint_conv(x: torch.Tensor, wt: torch.Tensor, bias: torch.Tensor, stride: int = 1, silu: bool = True) -> torch.Tensor:
    """One layer of ControlNet's hint encoder: x fp16 NHWC [n, h, w, cin] or — the first layer — fp32 NCHW [n, cin, h, w] -> fp16 NHWC
    [n, ho, wo, cout]; wt fp16 [cout, 9 cin] tap-major (repack_conv_weight), bias fp16 [cout]."""
    first = x.dtype == torch.float32
    n, cin, h, w = x.shape if first else (x.shape[0], x.shape[3], x.shape[1], x.shape[2])
    cout = wt.shape[0]
    y = torch.empty(n, (h - 1) // stride + 1, (w - 1) // stride + 1, cout, dtype=torch.float16, device=x.device)
    with torch.cuda.device(x.device):
        check(lib().ld_op_hint_conv(None if first else _p(x), _p(x) if first else None, n, h, w, cin, _p(wt), _p(bias), cout, stride, int(silu), _p(y),
                                    _stream()), "ld_op_hint_conv")
    return y


# ------------------------------------------------------------------ the `operations=` namespace (secondary seam)
# The reference builds every network from an injectable namespace (`operations=ops`: UNetModel1 LD.py:5338, ResBlock1
# 5207, SpatialTransformer 4179, CrossAttention 4005, FeedForward 3908; BaseModel picks `manual_cast` or
# `disable_weight_init`, LD.py:5809-5816).  The classes below have the torch constructor signatures and state-dict names
# (`weight`, `bias`) of LD.py:2342-2429 and run their forward on the HIP kernels.  Like `disable_weight_init` they do not
# initialise parameters (reset_parameters is a no-op, LD.py:2363); like `manual_cast` they accept any float input dtype
# and return it.  Feature maps keep torch's logical NCHW shape in channels_last memory, which *is* the kernels' NHWC
# layout, so a chain of these modules moves no data between ops.
import torch.nn as nn  # noqa: E402


def _to_f16_cl(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.float16).contiguous(memory_format=torch.channels_last)


class _NoInit:
    def reset_parameters(self):
        return None


class Linear(_NoInit, nn.Module):
    def __init__(self, in_features, out_features, bias=True, device=None, dtype=None):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.weight = nn.Parameter(torch.empty(out_features, in_features, device=device, dtype=dtype), requires_grad=False)
        self.bias = nn.Parameter(torch.empty(out_features, device=device, dtype=dtype), requires_grad=False) if bias else None

    def forward(self, x):
        w = self.weight.to(x.device, torch.float16)
        b = None if self.bias is None else self.bias.to(x.device, torch.float16)
        return linear(x.to(torch.float16).contiguous(), w.contiguous(), b).to(x.dtype)


class Conv2d(_NoInit, nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True,
                 padding_mode="zeros", device=None, dtype=None):
        super().__init__()
        k = kernel_size if isinstance(kernel_size, int) else kernel_size[0]
        st = stride if isinstance(stride, int) else stride[0]
        pd = padding if isinstance(padding, int) else padding[0]
        if k not in (1, 3) or pd != k // 2 or dilation not in (1, (1, 1)) or groups != 1 or padding_mode != "zeros":
            raise NotImplementedError("MI355X Conv2d: kernel 1 or 3 with padding k//2, no dilation / groups (all the SD1.x UNet and VAE use)")
        self.in_channels, self.out_channels, self.kernel_size, self.stride, self.padding = in_channels, out_channels, (k, k), (st, st), (pd, pd)
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, k, k, device=device, dtype=dtype), requires_grad=False)
        self.bias = nn.Parameter(torch.empty(out_channels, device=device, dtype=dtype), requires_grad=False) if bias else None
        self._packed = None

    def _weights(self, device):
        key = (self.weight.data_ptr(), self.weight._version, str(device))
        if self._packed is None or self._packed[0] != key:
            wp = repack_conv_weight(self.weight.detach().to(device))
            b = torch.zeros(self.out_channels, dtype=torch.float16, device=device) if self.bias is None else self.bias.detach().to(device, torch.float16)
            self._packed = (key, wp, b.contiguous())
        return self._packed[1], self._packed[2]

    def forward(self, x):
        n, c, h, w = x.shape
        xc = _to_f16_cl(x)
        wp, b = self._weights(x.device)
        y = conv2d(xc.permute(0, 2, 3, 1), wp, b, self.kernel_size[0], self.stride[0])          # a view: channels_last memory is NHWC
        return y.permute(0, 3, 1, 2).to(x.dtype)


class GroupNorm(_NoInit, nn.Module):
    def __init__(self, num_groups, num_channels, eps=1e-5, affine=True, device=None, dtype=None):
        super().__init__()
        if num_groups != 32 or not affine:
            raise NotImplementedError("MI355X GroupNorm: 32 groups, affine (Normalize, LD.py:3931-3939)")
        self.num_groups, self.num_channels, self.eps = num_groups, num_channels, eps
        self.weight = nn.Parameter(torch.empty(num_channels, device=device, dtype=dtype), requires_grad=False)
        self.bias = nn.Parameter(torch.empty(num_channels, device=device, dtype=dtype), requires_grad=False)

    def forward(self, x):
        xc = _to_f16_cl(x) if x.dim() == 4 else x.to(torch.float16).transpose(1, -1).contiguous()
        nhwc = xc.permute(0, 2, 3, 1) if x.dim() == 4 else xc
        y = group_norm(nhwc, self.weight.to(x.device, torch.float16), self.bias.to(x.device, torch.float16), self.eps)
        y = y.permute(0, 3, 1, 2) if x.dim() == 4 else y.transpose(1, -1)
        return y.to(x.dtype)


class LayerNorm(_NoInit, nn.Module):
    def __init__(self, normalized_shape, eps=1e-5, elementwise_affine=True, bias=True, device=None, dtype=None):
        super().__init__()
        c = normalized_shape if isinstance(normalized_shape, int) else normalized_shape[-1]
        if not isinstance(normalized_shape, int) and len(normalized_shape) != 1:
            raise NotImplementedError("MI355X LayerNorm: last-dimension normalisation")
        self.normalized_shape, self.eps = (c,), eps
        self.weight = nn.Parameter(torch.empty(c, device=device, dtype=dtype), requires_grad=False) if elementwise_affine else None
        self.bias = nn.Parameter(torch.empty(c, device=device, dtype=dtype), requires_grad=False) if elementwise_affine and bias else None

    def forward(self, x):
        c = self.normalized_shape[0]
        g = torch.ones(c, dtype=torch.float16, device=x.device) if self.weight is None else self.weight.to(x.device, torch.float16)
        b = torch.zeros(c, dtype=torch.float16, device=x.device) if self.bias is None else self.bias.to(x.device, torch.float16)
        return layer_norm(x.to(torch.float16).contiguous(), g, b, self.eps).to(x.dtype)


def conv_nd(dims, *args, **kwargs):
    """disable_weight_init.conv_nd (LD.py:2407-2412): only dims == 2 exists in the SD1.x networks."""
    if dims == 2:
        return Conv2d(*args, **kwargs)
    raise ValueError(f"unsupported dimensions: {dims}")


def optimized_attention(q, k, v, heads, mask=None):
    """The module-global attention function of LD.py:3966-3988: q [b,Lq,heads*d], k / v [b,Lk,heads*d] -> [b,Lq,heads*d]."""
    if mask is not None:
        raise NotImplementedError("MI355X optimized_attention: the SD1.x UNet passes no mask (LD.py:4028-4036)")
    f16 = lambda t: t.to(torch.float16).contiguous()
    return attention(f16(q), f16(k), f16(v), heads).to(q.dtype)
