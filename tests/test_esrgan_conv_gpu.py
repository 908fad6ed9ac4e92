"""GPU: the dense-block 3x3 convolution kernel alone (ld_op_esrgan_conv), element-wise against the fp64 convolution of the fp16 operands.

The kernel's tile is TILE_H x TILE_W = 16 x 32 output pixels per workgroup (esrgan.hip EG_TH / EG_TW); the image sizes below are under one
tile in both axes (5 x 7), the narrow tiles tiled_scale produces (8 x 32, 32 x 8), over the tile in both axes by a non-multiple (33 x 47:
3 x 2 workgroups, ragged last row and column), and a batch of two (9 x 11: an image's border rows must read zeros, not its neighbour).

Bound (derived as tests/errbound.py derives its own; nothing measured).  The kernel keeps fp32 from the accumulator to the single fp16
rounding at the store, so with acc the fp64 product sum and absdot = sum |a w|:
    pre  = acc + bias            e = c_acc(K) absdot + 2^-23 (|acc| + |pre|)        fp32 MFMA chain, one fp32 add
    v    = lrelu(pre, slope)     e <- e + 2^-23 |v|                                  Lipschitz constant 1, one fp32 multiply
    v    = s v + R  (each)       e <- |s| e + 2^-22 (|s v| + |v'|)                    fp32 multiply-add of an exact fp16 residual
    y    = round_fp16(v)         bound = 2^-11 |y_hat| + e + 2^-24
and the signed-bias criterion BIAS_TOL of errbound.check as for every route.
"""
import pytest
import torch

from errbound import TINY, U, c_acc, check, im2col
from lightdiffusion_amd._lib import ERR_ARG, ERR_SHAPE, OK, lib

pytestmark = pytest.mark.gpu
# the kernels of esrgan.hip this module holds (tests/test_errbound_cpu.py keeps the ledger; the end convolutions: tests/test_end_convs_gpu.py, the blend: tests/test_blend_gpu.py)
KERNELS = {"esrgan_conv_kernel": ["test_dense_conv_in_place", "test_conv5_residuals", "test_conv5_second_store", "test_upconv_nearest2x"]}

TILE_H, TILE_W = 16, 32
SIZES = [(1, 5, 7), (1, 8, 32), (1, 32, 8), (1, 33, 47), (2, 9, 11)]
F23 = 2.0 ** -23


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _repack(w_oihw):
    dst = torch.empty(w_oihw.shape[0], 9 * w_oihw.shape[1], dtype=torch.float16, device="cuda")
    src = w_oihw.contiguous()
    assert lib().ld_op_repack_conv(src.data_ptr(), 0, src.shape[0], src.shape[1], dst.data_ptr(), _stream()) == OK
    return dst


def dense_conv_ref(x, w_oihw, bias, slope=0.0, residuals=(), up=False):
    """y_hat [n*h*w][cout] (fp64) and the element bound of the module docstring.  x: NHWC fp16 (the channels the kernel reads)."""
    n, h, w, _ = x.shape
    out_hw = (2 * h, 2 * w) if up else None
    cols = im2col(x, 3, 1, out_hw)
    wm = w_oihw.double().reshape(w_oihw.shape[0], -1)
    acc, absdot = cols @ wm.t(), cols.abs() @ wm.abs().t()
    pre = acc + bias.double()
    e = c_acc(wm.shape[1]) * absdot + F23 * (acc.abs() + pre.abs())
    v = torch.where(pre > 0, pre, slope * pre) if slope != 0.0 else pre
    if slope != 0.0:
        e = e + F23 * v.abs()
    for s, r in residuals:
        nv = s * v + r.double().reshape(v.shape)
        e = abs(s) * e + 2 * F23 * ((s * v).abs() + nv.abs())
        v = nv
    return v, U * v.abs() + e + TINY


def _operands(cin, cout, n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, h, w, cin, generator=g).half().cuda()
    wt = (torch.randn(cout, cin, 3, 3, generator=g) / (3.0 * cin ** 0.5)).half().cuda()
    b = (0.1 * torch.randn(cout, generator=g)).half().cuda()
    return x, wt, b


def _call(x, ldx, cin, n, h, w, up, wr, b, y, ldy, c_off, cout, slope, r1=None, ldr1=0, s1=1.0, r2=None, ldr2=0, s2=1.0):
    p = lambda t: None if t is None else t.data_ptr()
    return lib().ld_op_esrgan_conv(p(x), ldx, cin, n, h, w, int(up), p(wr), p(b), p(y), ldy, c_off, cout, slope, p(r1), ldr1, s1, p(r2), ldr2, s2,
                                   _stream())


def _call_y2(x, ldx, cin, n, h, w, up, wr, b, y, ldy, c_off, cout, slope, r1=None, ldr1=0, s1=1.0, r2=None, ldr2=0, s2=1.0, y2=None, ldy2=0):
    """The same call with the second store (ld_op_esrgan_conv_y2)."""
    p = lambda t: None if t is None else t.data_ptr()
    return lib().ld_op_esrgan_conv_y2(p(x), ldx, cin, n, h, w, int(up), p(wr), p(b), p(y), ldy, c_off, cout, slope, p(r1), ldr1, s1, p(r2), ldr2, s2,
                                      p(y2), ldy2, _stream())


@pytest.mark.parametrize("n,h,w", SIZES)
@pytest.mark.parametrize("cin", [64, 96, 128, 160, 192])
def test_dense_conv_in_place(cin, n, h, w):
    """conv k of a block: reads channels [0, cin) of the dense buffer, writes LeakyReLU(0.2) output into [cin, cin + 32) of the SAME
    buffer; every other channel keeps its sentinel bit pattern.  The pitch is the network's 192; cin = 192 has no room behind it there
    and runs in a pitch-224 buffer."""
    ld = max(192, cin + 32)
    x, wt, b = _operands(cin, 32, n, h, w, 100 + cin + h)
    buf = torch.full((n, h, w, ld), -7.25, dtype=torch.float16, device="cuda")
    buf.view(torch.int16)[..., 1::2] += 1                       # two sentinel patterns, alternating by channel
    buf[..., :cin] = x
    before = buf.clone()
    assert _call(buf, ld, cin, n, h, w, False, _repack(wt), b, buf, ld, cin, 32, 0.2) == OK
    assert lib().ld_op_last_kernel().decode() == "esrgan_conv_kernel<32>"
    torch.cuda.synchronize()
    keep = torch.ones(ld, dtype=torch.bool, device="cuda")
    keep[cin:cin + 32] = False
    assert torch.equal(buf.view(torch.int16)[..., keep], before.view(torch.int16)[..., keep]), "channels outside [c_off, c_off + 32) changed"
    ref, bound = dense_conv_ref(x, wt, b, 0.2)
    check(buf[..., cin:cin + 32].reshape(-1, 32), ref, bound, f"dense conv {cin}->32 at {n}x{h}x{w}", image_rows=h * w, width=w)


@pytest.mark.parametrize("n,h,w", SIZES)
@pytest.mark.parametrize("two", [False, True])
def test_conv5_residuals(two, n, h, w):
    """conv5: 192 -> 64, x5 * 0.2 + x (R1 = the block's input, the first 64 channels of the pitch-192 buffer), and with the RRDB's
    outer out * 0.2 + x as R2."""
    x, wt, b = _operands(192, 64, n, h, w, 200 + h + int(two))
    r2 = torch.randn(n, h, w, 64, generator=torch.Generator().manual_seed(5)).half().cuda()
    y = torch.zeros(n, h, w, 192, dtype=torch.float16, device="cuda")
    st = _call(x, 192, 192, n, h, w, False, _repack(wt), b, y, 192, 0, 64, 0.0, x, 192, 0.2, r2 if two else None, 64, 0.2)
    assert st == OK and lib().ld_op_last_kernel().decode() == "esrgan_conv_kernel<64>"
    res = [(0.2, x[..., :64])] + ([(0.2, r2)] if two else [])
    ref, bound = dense_conv_ref(x, wt, b, 0.0, res)
    check(y[..., :64].reshape(-1, 64), ref, bound, f"conv5 R1{'+R2' if two else ''} at {n}x{h}x{w}", image_rows=h * w, width=w)
    assert not bool(y[..., 64:].any())


@pytest.mark.parametrize("n,h,w", SIZES)
def test_conv5_second_store(n, h, w):
    """conv5 of an RRDB's third block: R1 + R2 and the second store y2 (halo_conv.h: the same packed values at pitch ldy2) — first into a
    buffer of its own, then over R2 itself, the executor's aliasing (r2 == y2 == the RRDB's input): every lane reads its R2 elements before it
    overwrites them, so the result is the same y and R2 holds y afterwards."""
    x, wt, b = _operands(192, 64, n, h, w, 400 + h)
    wr = _repack(wt)
    r2 = torch.randn(n, h, w, 64, generator=torch.Generator().manual_seed(6)).half().cuda()
    y = torch.zeros(n, h, w, 192, dtype=torch.float16, device="cuda")
    y2 = torch.full((n, h, w, 64), -7.25, dtype=torch.float16, device="cuda")
    st = _call_y2(x, 192, 192, n, h, w, False, wr, b, y, 192, 0, 64, 0.0, x, 192, 0.2, r2, 64, 0.2, y2, 64)
    assert st == OK and lib().ld_op_last_kernel().decode() == "esrgan_conv_kernel<64>"
    ref, bound = dense_conv_ref(x, wt, b, 0.0, [(0.2, x[..., :64]), (0.2, r2)])
    check(y[..., :64].reshape(-1, 64), ref, bound, f"conv5 R1+R2 with y2 at {n}x{h}x{w}", image_rows=h * w, width=w)
    assert torch.equal(y2.view(torch.int16), y[..., :64].contiguous().view(torch.int16)), "y2 is not y[..., :64] bit for bit"
    assert not bool(y[..., 64:].any())
    ya = torch.zeros_like(y)
    alias = r2.clone()
    assert _call_y2(x, 192, 192, n, h, w, False, wr, b, ya, 192, 0, 64, 0.0, x, 192, 0.2, alias, 64, 0.2, alias, 64) == OK
    assert torch.equal(ya.view(torch.int16), y.view(torch.int16)), "y2 == r2 changed y"
    assert torch.equal(alias.view(torch.int16), y2.view(torch.int16)), "r2 does not hold y after the aliased call"


@pytest.mark.parametrize("n,h,w", SIZES)
def test_upconv_nearest2x(n, h, w):
    """upconv_block: the source is (h, w), the output (2h, 2w): halo pixel (y, x) <- source (y >> 1, x >> 1); LeakyReLU 0.2."""
    x, wt, b = _operands(64, 64, n, h, w, 300 + h)
    y = torch.zeros(n, 2 * h, 2 * w, 64, dtype=torch.float16, device="cuda")
    assert _call(x, 64, 64, n, 2 * h, 2 * w, True, _repack(wt), b, y, 64, 0, 64, 0.2) == OK
    assert lib().ld_op_last_kernel().decode() == "esrgan_conv_kernel<64,up>"
    ref, bound = dense_conv_ref(x, wt, b, 0.2, up=True)
    check(y.reshape(-1, 64), ref, bound, f"upconv 64->64 at {n}x{h}x{w}", image_rows=4 * h * w, width=2 * w)


def test_arguments_are_checked_before_any_launch():
    x, wt, b = _operands(64, 32, 1, 5, 7, 1)
    wr = _repack(wt)
    buf = torch.zeros(1, 5, 7, 192, dtype=torch.float16, device="cuda")
    y = torch.zeros(1, 5, 7, 64, dtype=torch.float16, device="cuda")
    call = lambda **k: _call(**{**dict(x=buf, ldx=192, cin=64, n=1, h=5, w=7, up=False, wr=wr, b=b, y=y, ldy=64, c_off=0, cout=32, slope=0.2), **k})
    assert call() == OK
    assert call(y=buf, ldy=192, c_off=32) == ERR_ARG and lib().ld_op_last_kernel().decode() == ""     # aliased, c_off < cin
    assert call(y=buf, ldy=192, c_off=0) == ERR_ARG
    assert call(y=buf[:, :, :, 8:], ldy=192, c_off=64) == ERR_ARG                                      # overlapping, not the same buffer
    assert call(x=None) == ERR_ARG and call(y=None) == ERR_ARG and call(wr=None) == ERR_ARG
    assert call(cin=32) == ERR_SHAPE and call(cin=80) == ERR_SHAPE and call(cin=224, ldx=224) == ERR_SHAPE
    assert call(cout=16) == ERR_SHAPE and call(cout=48) == ERR_SHAPE
    assert call(ldx=32) == ERR_SHAPE and call(c_off=40) == ERR_SHAPE and call(ldy=60) == ERR_SHAPE
    assert call(h=0) == ERR_SHAPE and call(up=True) == ERR_SHAPE                                      # odd output size behind a 2x upsampling
    torch.cuda.synchronize()


def test_second_store_arguments_are_checked_before_any_launch():
    x, wt, b = _operands(64, 32, 1, 5, 7, 1)
    wr = _repack(wt)
    buf = torch.zeros(1, 5, 7, 192, dtype=torch.float16, device="cuda")
    y = torch.zeros(1, 5, 7, 64, dtype=torch.float16, device="cuda")
    y2 = torch.zeros(1, 5, 7, 64, dtype=torch.float16, device="cuda")
    call = lambda **k: _call_y2(**{**dict(x=buf, ldx=192, cin=64, n=1, h=5, w=7, up=False, wr=wr, b=b, y=y, ldy=64, c_off=0, cout=32, slope=0.2), **k})
    assert call() == OK and call(y2=y2, ldy2=64) == OK and call(y2=y2, ldy2=32) == OK
    assert call(y2=y2, ldy2=24) == ERR_SHAPE and call(y2=y2, ldy2=36) == ERR_SHAPE                      # ldy2 < cout; ldy2 & 7
    assert call(y2=buf, ldy2=192) == ERR_ARG and call(y2=buf[:, :, :, 64:], ldy2=192) == ERR_ARG         # y2 overlapping x
    assert lib().ld_op_last_kernel().decode() == ""
    torch.cuda.synchronize()
