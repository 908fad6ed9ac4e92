"""GPU: ControlNet's two kernels (csrc/control/control.hip) through lightdiffusion_amd.ops.
  control add   BITWISE against the expression in torch on the host, (t.float() + strength * r.float()).half(): IEEE fp32 product and sum and the
                round-to-nearest conversion are the same bits on either side (the kernel uses __fmul_rn / __fadd_rn: no FMA).  Segments whose
                size per sample is and is not a multiple of the 8-half vector, r_n = 1 against n = 3, r_n = n, the CFG pair's r_n = n / 2, strength 0
                (the input bits: inputs are seeded randn, no -0.0 among them), 16 segments in one launch, pointers that are not 16-byte aligned
                (the scalar path), a captured launch.
  hint conv     element-wise against an fp64 convolution of the same fp16 values, bound built from tests/errbound.py:
                    e_pre = c_acc(9 Cin) sum|a w| + 2^-23 (|acc| + |pre|)          fp32 chain, the fp32 bias add
                    bound = U |y| + L e_pre + SILU_F32 |y| + TINY                  L = L_ACT with SiLU (1 without), one fp16 rounding at the store
                SILU_F32 = 2^-21 + 2^-23 |pre|: silu_f in fp32 — the exponent's argument is rounded (relative 2^-24 of |pre| on e^-pre), v_exp_f32 and
                the division within an ulp or two each.  And the signed-bias statistic of errbound.check.  Shapes: 16 x 24 and 8 x 8 images, stride 1
                and 2, batch 1 and 3, every (Cin, Cout) pair of the encoder's chain at tiny and SD1.5 width, and the fp32-NCHW first layer.
KERNELS names the tests that hold each kernel; tests/test_control_ledger_cpu.py keeps that ledger."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import errbound as EB                                          # noqa: E402
from lightdiffusion_amd import ops                             # noqa: E402
from lightdiffusion_amd import weights as W                    # noqa: E402
from lightdiffusion_amd._lib import ERR_ARG, ERR_SHAPE, LDError   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

KERNELS = {
    "control_add_kernel": ("test_control_add", "test_control_add_sixteen_segments", "test_control_add_unaligned_takes_the_scalar_path",
                           "test_control_add_is_capturable"),
    "hint_conv_kernel": ("test_hint_conv", "test_hint_conv_first_layer"),
}


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int16), b.view(torch.int16))


def expr(t, r, strength):
    """the expression, on the host; r [r_n, ...] repeats over t's batch as sample s % r_n"""
    rep = t.shape[0] // r.shape[0]
    rr = r.float().repeat((rep,) + (1,) * (r.dim() - 1))
    return (t.float() + strength * rr).half()


def pair(g, n, r_n, shape, scale=3.0):
    return (torch.randn((n,) + shape, generator=g) * scale).half(), (torch.randn((r_n,) + shape, generator=g) * scale).half()


# per-sample sizes: 960 and 64 * 4 * 4 (multiples of 8), 105 and 7 (not)
SHAPES = {"vector": [(5, 3, 64), (4, 4, 64)], "scalar": [(7, 3, 5), (7,)], "mixed": [(5, 3, 64), (7, 3, 5)]}


@pytest.mark.parametrize("kind", list(SHAPES))
@pytest.mark.parametrize("n,r_n", [(3, 1), (3, 3), (4, 2), (1, 1)])
@pytest.mark.parametrize("strength", [1.0, 0.0, 0.7, -1.25])
def test_control_add(kind, n, r_n, strength):
    g = torch.Generator().manual_seed(100 * n + 10 * r_n + len(kind))
    ts, rs = zip(*[pair(g, n, r_n, s) for s in SHAPES[kind]])
    want = [expr(t, r, strength) for t, r in zip(ts, rs)]
    dt, dr = [t.to(DEV) for t in ts], [r.to(DEV) for r in rs]
    keep = [r.clone() for r in dr]
    ops.control_add_(dt, dr, strength)
    for t, t0, w, r, r0 in zip(dt, ts, want, dr, keep):
        assert same_bits(t.cpu(), w)
        assert torch.equal(r, r0)                                  # the residual is read only
        if strength == 0.0:
            assert same_bits(t.cpu(), t0)                          # strength 0: the input bits
        else:
            assert not same_bits(t.cpu(), t0)


def test_control_add_sixteen_segments():
    g = torch.Generator().manual_seed(16)
    shapes = [(1 + i % 3, 2 + i % 5, 8 * (1 + i % 4)) for i in range(16)]
    ts, rs = zip(*[pair(g, 2, 1, s) for s in shapes])
    want = [expr(t, r, 0.5) for t, r in zip(ts, rs)]
    dt = [t.to(DEV) for t in ts]
    ops.control_add_(dt, [r.to(DEV) for r in rs], 0.5)
    assert all(same_bits(t.cpu(), w) for t, w in zip(dt, want))
    with pytest.raises(LDError) as e:                              # 17 do not fit one launch
        ops.control_add_(dt + dt[:1], [r.to(DEV) for r in rs] + [rs[0].to(DEV)], 0.5)
    assert e.value.status == ERR_SHAPE
    with pytest.raises(LDError) as e:                              # r_n does not divide n
        ops.control_add_([torch.zeros(3, 8, dtype=torch.float16, device=DEV)], [torch.zeros(2, 8, dtype=torch.float16, device=DEV)], 1.0, n=3, r_n=2)
    assert e.value.status == ERR_SHAPE


def test_control_add_unaligned_takes_the_scalar_path():
    """per = 64 is a multiple of 8, but the pointers sit 2 bytes off a 16-byte boundary: single halves, the same bits"""
    g = torch.Generator().manual_seed(5)
    t, r = pair(g, 3, 1, (64,))
    bt, br = torch.zeros(3 * 64 + 1, dtype=torch.float16, device=DEV), torch.zeros(64 + 1, dtype=torch.float16, device=DEV)
    bt[1:].copy_(t.flatten())
    br[1:].copy_(r.flatten())
    vt, vr = bt[1:].view(3, 64), br[1:].view(1, 64)
    assert vt.data_ptr() % 16 == 2
    ops.control_add_([vt], [vr], 0.75)
    assert same_bits(vt.cpu(), expr(t, r, 0.75)) and float(bt[0]) == 0.0 and float(br[0]) == 0.0


def test_control_add_is_capturable():
    g = torch.Generator().manual_seed(6)
    t, r = pair(g, 2, 2, (4, 4, 16))
    dt, dr = t.to(DEV), r.to(DEV)
    ops.control_add_([dt], [dr], 0.5)                               # warm-up outside capture
    dt.copy_(t)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        ops.control_add_([dt], [dr], 0.5)
    dt.copy_(t)
    graph.replay()
    assert same_bits(dt.cpu(), expr(t, r, 0.5))


# ------------------------------------------------------------------ the hint encoder's convolution
SILU_F32 = lambda pre: 2.0 ** -21 + 2.0 ** -23 * pre.abs()

CHAIN = (3,) + W.HINT_CHANNELS
PAIRS = sorted({(CHAIN[i], CHAIN[i + 1]) for i in range(1, 7)} | {(256, 64), (256, 320)})      # every fp16 layer, at tiny and SD1.5 width


def hint_ref(a_nhwc, w_oihw, bias, stride, silu):
    """a_nhwc: the fp16 VALUES the kernel contracts, as a tensor on the device -> (y_hat, bound) [n ho wo][cout], fp64"""
    cols = EB.im2col(a_nhwc, 3, stride)
    wm = w_oihw.double().reshape(w_oihw.shape[0], -1)
    acc, absdot = cols @ wm.t(), cols.abs() @ wm.abs().t()
    pre = acc + bias.double()
    e_pre = EB.c_acc(9 * a_nhwc.shape[-1]) * absdot + 2.0 ** -23 * (acc.abs() + pre.abs())
    if silu:
        y = pre * torch.sigmoid(pre)
        return y, EB.U * y.abs() + EB.L_ACT * e_pre + SILU_F32(pre) * y.abs() + EB.TINY
    return pre, EB.U * pre.abs() + e_pre + EB.TINY


def weights_of(g, cin, cout):
    w = (torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5).half().to(DEV)
    b = (torch.randn(cout, generator=g) * 0.5).half().to(DEV)
    return w, ops.repack_conv_weight(w), b


def held(y, ref, bound, what, width):
    n_eff = EB.independent_roundings(ref)
    return EB.check(y.reshape(ref.shape), ref, bound, what, image_rows=ref.shape[0] // y.shape[0], width=width, bias_extra=EB.rtn_noise(n_eff))


@pytest.mark.parametrize("hw", [(16, 24), (8, 8)])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("cin,cout", PAIRS)
def test_hint_conv(hw, stride, n, cin, cout):
    g = torch.Generator().manual_seed(cin * 1000 + cout + stride)
    h, w = hw
    x = torch.randn(n, h, w, cin, generator=g).half().to(DEV)
    wt, packed, b = weights_of(g, cin, cout)
    silu = cout not in (64, 320) or cin != 256                     # the encoder's last layer has no activation
    y = ops.hint_conv(x, packed, b, stride=stride, silu=silu)
    assert tuple(y.shape) == (n, (h - 1) // stride + 1, (w - 1) // stride + 1, cout)
    ref, bound = hint_ref(x, wt, b, stride, silu)
    held(y, ref, bound, f"hint conv {cin}->{cout} s{stride} n{n} {h}x{w}", y.shape[2])


@pytest.mark.parametrize("hw", [(16, 24), (8, 8)])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("n", [1, 3])
def test_hint_conv_first_layer(hw, stride, n):
    """the fp32 NCHW image, every sample rounded to fp16 once (reproduced exactly: no allowance)"""
    g = torch.Generator().manual_seed(33 + stride)
    h, w = hw
    img = torch.rand(n, 3, h, w, generator=g).to(DEV)
    wt, packed, b = weights_of(g, 3, 16)
    y = ops.hint_conv(img, packed, b, stride=stride, silu=True)
    ref, bound = hint_ref(img.half().permute(0, 2, 3, 1).contiguous(), wt, b, stride, True)
    held(y, ref, bound, f"hint first s{stride} n{n} {h}x{w}", y.shape[2])


def test_hint_conv_refuses_what_it_does_not_run():
    g = torch.Generator().manual_seed(1)
    _, packed, b = weights_of(g, 16, 16)
    x = torch.zeros(1, 8, 8, 16, dtype=torch.float16, device=DEV)
    with pytest.raises(LDError) as e:
        ops.hint_conv(x, packed, b, stride=3)
    assert e.value.status == ERR_SHAPE
    with pytest.raises(LDError) as e:                              # an fp16 input of 12 channels: no 16-byte channel chunks
        ops.hint_conv(torch.zeros(1, 8, 8, 12, dtype=torch.float16, device=DEV), packed, b)
    assert e.value.status == ERR_SHAPE
    assert ERR_ARG != ERR_SHAPE
