"""GPU: TAESD's 64 -> 64 convolution alone (ld_op_taesd_conv), element-wise against the fp64 convolution of the fp16 operands.

The kernel is the halo-tile main loop of the ESRGAN dense-block kernel (csrc/halo_conv.h, 16 x 32 output pixels per workgroup) under
TAESD's epilogue.  Sizes as in tests/test_esrgan_conv_gpu.py: under one tile in both axes (5 x 7), over the tile in both axes by a
non-multiple (33 x 47: 3 x 2 workgroups, ragged last row and column), and a batch of two (9 x 11: an image's border rows must read zeros,
not its neighbour).  Without `up` they are the output size; with `up` they are the SOURCE size and the output is (2h, 2w), as an
upsampling needs an even output.

Bound (derived as tests/errbound.py derives its own; nothing measured).  The kernel keeps fp32 from the accumulator to the single fp16
rounding at the store, so with acc the fp64 product sum and absdot = sum |a w|:
    pre  = acc + bias            e = c_acc(576) absdot + 2^-23 (|acc| + |pre|)      fp32 MFMA chain, one fp32 add
    v    = pre + R               e <- e + 2^-23 |v|                                  one fp32 add of an exact fp16 residual
    v    = relu(v)                                                                    exact, Lipschitz constant 1
    y    = round_fp16(v)         bound = 2^-11 |y_hat| + e + 2^-24
and the signed-bias criterion BIAS_TOL of errbound.check as for every route.
"""
import itertools

import pytest
import torch

from errbound import TINY, U, c_acc, check, im2col
from lightdiffusion_amd._lib import ERR_ARG, ERR_SHAPE, OK, lib

pytestmark = pytest.mark.gpu
# the kernel of taesd.hip this module holds (tests/test_errbound_cpu.py keeps the ledger; the end convolutions: tests/test_end_convs_gpu.py)
KERNELS = {"taesd_conv_kernel": ["test_conv_64_to_64"]}

SIZES = [(1, 5, 7), (1, 33, 47), (2, 9, 11)]
F23 = 2.0 ** -23


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _repack(w_oihw):
    dst = torch.empty(w_oihw.shape[0], 9 * w_oihw.shape[1], dtype=torch.float16, device="cuda")
    src = w_oihw.contiguous()
    assert lib().ld_op_repack_conv(src.data_ptr(), 0, src.shape[0], src.shape[1], dst.data_ptr(), _stream()) == OK
    return dst


def taesd_conv_ref(x, w_oihw, bias, residual, relu, up):
    """y_hat [n*h*w][64] (fp64) and the element bound of the module docstring.  x: NHWC fp16."""
    n, h, w, _ = x.shape
    cols = im2col(x, 3, 1, (2 * h, 2 * w) if up else None)
    wm = w_oihw.double().reshape(w_oihw.shape[0], -1)
    assert wm.shape[1] == 576
    acc, absdot = cols @ wm.t(), cols.abs() @ wm.abs().t()
    pre = acc + (bias.double() if bias is not None else 0.0)
    e = c_acc(576) * absdot + F23 * (acc.abs() + pre.abs())
    v = pre
    if residual is not None:
        v = pre + residual.double().reshape(pre.shape)
        e = e + F23 * v.abs()
    if relu:
        v = v.clamp_min(0.0)
    return v, U * v.abs() + e + TINY


def _call(x, n, h, w, up, wr, b, r, relu, y):
    p = lambda t: None if t is None else t.data_ptr()
    return lib().ld_op_taesd_conv(p(x), n, h, w, int(up), p(wr), p(b), p(r), int(relu), p(y), _stream())


@pytest.mark.parametrize("bias,residual,relu", list(itertools.product([False, True], repeat=3)))
@pytest.mark.parametrize("up", [False, True])
@pytest.mark.parametrize("n,h,w", SIZES)
def test_conv_64_to_64(n, h, w, up, bias, residual, relu):
    g = torch.Generator().manual_seed(1000 + 8 * h + 4 * int(bias) + 2 * int(residual) + int(relu) + 16 * int(up))
    x = torch.randn(n, h, w, 64, generator=g).half().cuda()
    wt = (torch.randn(64, 64, 3, 3, generator=g) / 24.0).half().cuda()
    b = (0.1 * torch.randn(64, generator=g)).half().cuda() if bias else None
    oh, ow = (2 * h, 2 * w) if up else (h, w)
    r = torch.randn(n, oh, ow, 64, generator=g).half().cuda() if residual else None
    y = torch.full((n, oh, ow, 64), -7.25, dtype=torch.float16, device="cuda")
    assert _call(x, n, oh, ow, up, _repack(wt), b, r, relu, y) == OK
    assert lib().ld_op_last_kernel().decode() == ("taesd_conv_kernel<up>" if up else "taesd_conv_kernel")
    ref, bound = taesd_conv_ref(x, wt, b, r, relu, up)
    if relu:
        assert float(y.min()) >= 0.0
    # half of a ReLU output is exactly zero: the signed-bias statistic keeps the elements above its floor, as for every route
    check(y.reshape(-1, 64), ref, bound, f"taesd conv{' up' if up else ''} bias={bias} residual={residual} relu={relu} at {n}x{oh}x{ow}",
          image_rows=oh * ow, width=ow)


def test_arguments_are_checked_before_any_launch():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(1, 6, 8, 64, generator=g).half().cuda()
    wr = _repack((torch.randn(64, 64, 3, 3, generator=g) / 24.0).half().cuda())
    b = torch.zeros(64, dtype=torch.float16, device="cuda")
    y = torch.zeros(1, 6, 8, 64, dtype=torch.float16, device="cuda")
    big = torch.zeros(1, 12, 16, 64, dtype=torch.float16, device="cuda")
    call = lambda **k: _call(**{**dict(x=x, n=1, h=6, w=8, up=False, wr=wr, b=b, r=None, relu=1, y=y), **k})
    assert call() == OK
    assert call(x=None) == ERR_ARG and call(y=None) == ERR_ARG and call(wr=None) == ERR_ARG
    assert lib().ld_op_last_kernel().decode() == ""
    assert call(y=x) == ERR_ARG                                            # a tile's halo is another tile's output
    assert call(y=x.view(-1)[64:]) == ERR_ARG                              # overlapping, not the same buffer
    assert call(r=y) == ERR_ARG                                            # the residual is the output
    assert call(r=x) == OK                                                 # ... the input is fine (a Block's skip)
    assert call(h=0) == ERR_SHAPE and call(n=0) == ERR_SHAPE and call(w=-1) == ERR_SHAPE
    assert call(up=True, h=5, w=8, y=big) == ERR_SHAPE                     # odd output size behind a 2x upsampling
    assert call(up=True, h=12, w=16, y=big) == OK
    torch.cuda.synchronize()
