"""GPU: the masked sampler step's two fp32 blend kernels (csrc/inpaint/inpaint.hip) through lightdiffusion_amd.ops, held BITWISE against their
expression evaluated operation by operation in torch fp32 on the same inputs (on the host: IEEE fp32 products, sums and differences are the same
bits on either side).  No tolerance: the unit is built without contraction, as detail_image.hip is.
  in    out = x * m + (noise * sigma[b] + latent) * (1 - m)
  out   den = den * m + latent * (1 - m), in place
Shapes: one element per plane; an odd plane with no vector alignment and an odd batch; aligned planes (the float4 path); more than one block with
a tail.  Each with the mask as [1,1,h,w], [B,1,h,w] and [B,C,h,w] (and [1,C,h,w]); sigma differs per sample; mask values include exact 0 and 1.
KERNELS names the tests that hold each kernel; tests/test_inpaint_ledger_cpu.py keeps that ledger."""
import pytest
import torch

from lightdiffusion_amd import ops
from lightdiffusion_amd._lib import ERR_ARG, ERR_SHAPE, OK, lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

KERNELS = {
    "inpaint_blend_in_kernel": ("test_blend_in", "test_blend_in_mask_of_ones_and_zeros", "test_blend_in_out_may_be_x"),
    "inpaint_blend_out_kernel": ("test_blend_out", "test_blend_out_mask_of_ones_and_zeros"),
}

SHAPES = [(1, 4, 1, 1), (3, 4, 5, 7), (2, 4, 16, 24), (2, 4, 33, 65)]
MASKS = ["11", "B1", "BC", "1C"]


def mask_shape(shape, kind):
    b, c, h, w = shape
    return (b if kind[0] == "B" else 1, c if kind[1] == "C" else 1, h, w)


def inputs(shape, kind, seed=0):
    """x, mask, latent, noise, sigma on the host: normal values, a mask with exact zeros, exact ones and values in between, a sigma per sample"""
    g = torch.Generator().manual_seed(1000 * seed + shape[0] * shape[2] * shape[3])
    x, lat, noise = (torch.randn(shape, generator=g) * s for s in (5.0, 1.0, 1.0))
    m = torch.rand(mask_shape(shape, kind), generator=g)
    pick = torch.rand(m.shape, generator=g)
    m = torch.where(pick < 0.25, torch.zeros_like(m), torch.where(pick > 0.75, torch.ones_like(m), m))
    if m.numel() >= 8:
        assert bool((m == 0).any()) and bool((m == 1).any()) and bool(((m > 0) & (m < 1)).any())
    sigma = torch.tensor([14.6146, 0.0292, 1.7])[: shape[0]].contiguous()
    return x, m, lat, noise, sigma


def expr_in(x, m, lat, noise, sigma):
    keep = x * m
    noised = noise * sigma.view(-1, 1, 1, 1)
    noised = noised + lat
    return keep + noised * (1.0 - m)


def expr_out(den, m, lat):
    return den * m + lat * (1.0 - m)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def dev(*ts):
    return [t.to(DEV) for t in ts]


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("shape", SHAPES)
def test_blend_in(shape, kind):
    x, m, lat, noise, sigma = inputs(shape, kind)
    dx, dm, dl, dn, ds = dev(x, m, lat, noise, sigma)
    got = ops.inpaint_in(dx, dm, dl, dn, ds)
    assert got.data_ptr() != dx.data_ptr() and got.is_contiguous() and tuple(got.shape) == shape
    want = expr_in(x, m, lat, noise, sigma)
    assert same_bits(got.cpu(), want)
    assert same_bits(got.cpu(), expr_in(dx, dm, dl, dn, ds).cpu()), "and the same expression in torch on the device"
    for before, after in ((x, dx), (m, dm), (lat, dl), (noise, dn), (sigma, ds)):
        assert same_bits(after.cpu(), before), "the inputs are read only"
    if shape[0] > 1:
        assert not same_bits(got[0].cpu(), expr_in(x[:1], m[:1], lat[:1], noise[:1], sigma[1:2])), "each sample takes its own sigma"


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("shape", SHAPES)
def test_blend_out(shape, kind):
    den, m, lat, _, _ = inputs(shape, kind, seed=1)
    dd, dm, dl = dev(den, m, lat)
    assert ops.inpaint_out_(dd, dm, dl) is dd
    assert same_bits(dd.cpu(), expr_out(den, m, lat))
    assert same_bits(dd.cpu(), expr_out(*dev(den, m, lat)).cpu())
    assert same_bits(dm.cpu(), m) and same_bits(dl.cpu(), lat)


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("shape", SHAPES)
def test_blend_in_mask_of_ones_and_zeros(shape, kind):
    x, m, lat, noise, sigma = inputs(shape, kind, seed=2)
    dx, dm, dl, dn, ds = dev(x, m, lat, noise, sigma)
    assert same_bits(ops.inpaint_in(dx, torch.ones_like(dm), dl, dn, ds).cpu(), x), "m == 1 returns x"
    noised = noise * sigma.view(-1, 1, 1, 1) + lat
    assert same_bits(ops.inpaint_in(dx, torch.zeros_like(dm), dl, dn, ds).cpu(), noised), "m == 0 returns noise * sigma + latent"


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("shape", SHAPES)
def test_blend_out_mask_of_ones_and_zeros(shape, kind):
    den, m, lat, _, _ = inputs(shape, kind, seed=3)
    dd, dm, dl = dev(den, m, lat)
    assert same_bits(ops.inpaint_out_(dd.clone(), torch.ones_like(dm), dl).cpu(), den), "m == 1 returns den"
    assert same_bits(ops.inpaint_out_(dd.clone(), torch.zeros_like(dm), dl).cpu(), lat), "m == 0 returns latent"


@pytest.mark.parametrize("shape", SHAPES)
def test_blend_in_out_may_be_x(shape):
    x, m, lat, noise, sigma = inputs(shape, "B1", seed=4)
    dx, dm, dl, dn, ds = dev(x, m, lat, noise, sigma)
    assert ops.inpaint_in(dx, dm, dl, dn, ds, out=dx) is dx
    assert same_bits(dx.cpu(), expr_in(x, m, lat, noise, sigma))
    other = torch.full(shape, -7.0, device=DEV)
    assert ops.inpaint_in(dev(x)[0], dm, dl, dn, ds, out=other) is other and same_bits(other.cpu(), dx.cpu())


def test_unaligned_pointers_take_the_scalar_path():
    """Planes of 16 x 24 floats that start 4 bytes off a 16-byte boundary (views into a larger buffer, handed to the raw entry): the float4 path
    is for aligned rows only, and the result is the same bits."""
    shape = (2, 4, 16, 24)
    x, m, lat, noise, sigma = inputs(shape, "BC", seed=5)
    n = x.numel()

    def off_by_one(t):
        buf = torch.zeros(t.numel() + 4, device=DEV)
        buf[1:1 + t.numel()] = t.flatten().to(DEV)
        return buf, buf.data_ptr() + 4
    (bx, px), (bm, pm), (bl, pl), (bn, pn) = (off_by_one(t) for t in (x, m, lat, noise))
    out = torch.full((n + 4,), -7.0, device=DEV)
    ds = sigma.to(DEV)
    assert px % 16 == 4
    st = lib().ld_op_inpaint_in(px, pm, pl, pn, ds.data_ptr(), out.data_ptr() + 4, 2, 4, 16 * 24, 2, 4, torch.cuda.current_stream().cuda_stream)
    assert st == OK
    assert same_bits(out[1:1 + n].view(shape).cpu(), expr_in(x, m, lat, noise, sigma))
    assert out[0].item() == -7.0 and bool((out[1 + n:] == -7.0).all()), "nothing outside the tensor is written"
    st = lib().ld_op_inpaint_out(px, pm, pl, 2, 4, 16 * 24, 2, 4, torch.cuda.current_stream().cuda_stream)
    assert st == OK
    assert same_bits(bx[1:1 + n].view(shape).cpu(), expr_out(x, m, lat))
    assert bx[0].item() == 0.0 and bool((bx[1 + n:] == 0.0).all())


def test_blends_are_capturable():
    """Stream-ordered, no allocation with `out` given, no host read: both launches go into a hipGraph, and a replay reads the sigma that is in device
    memory then."""
    shape = (2, 4, 16, 24)
    x, m, lat, noise, sigma = inputs(shape, "B1", seed=6)
    dx, dm, dl, dn, ds = dev(x, m, lat, noise, sigma)
    out = torch.zeros(shape, device=DEV)
    den = torch.zeros(shape, device=DEV)
    ops.inpaint_in(dx, dm, dl, dn, ds, out=out)            # warm-up outside capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        ops.inpaint_in(dx, dm, dl, dn, ds, out=out)
        ops.inpaint_out_(den, dm, dl)
    sigma2 = torch.tensor([0.5, 9.0])
    ds.copy_(sigma2)
    den.copy_(x)
    g.replay()
    torch.cuda.synchronize()
    assert same_bits(out.cpu(), expr_in(x, m, lat, noise, sigma2))
    assert same_bits(den.cpu(), expr_out(x, m, lat))


def test_rejections():
    shape = (3, 4, 5, 7)
    x, m, lat, noise, sigma = inputs(shape, "B1", seed=7)
    dx, dm, dl, dn, ds = dev(x, m, lat, noise, sigma)
    out = torch.full(shape, -7.0, device=DEV)
    raw_in = lambda px, pm, pl, pn, ps, po, B=3, C=4, HW=35, Bm=3, Cm=1: lib().ld_op_inpaint_in(px, pm, pl, pn, ps, po, B, C, HW, Bm, Cm, None)
    raw_out = lambda pd, pm, pl, B=3, C=4, HW=35, Bm=3, Cm=1: lib().ld_op_inpaint_out(pd, pm, pl, B, C, HW, Bm, Cm, None)
    p = [t.data_ptr() for t in (dx, dm, dl, dn, ds, out)]
    for i in range(6):                                                  # a null pointer, whichever it is
        assert raw_in(*[None if j == i else v for j, v in enumerate(p)]) == ERR_ARG, i
    po = [out.data_ptr(), dm.data_ptr(), dl.data_ptr()]
    for i in range(3):
        assert raw_out(*[None if j == i else v for j, v in enumerate(po)]) == ERR_ARG, i
    assert raw_in(*p, Bm=2) == ERR_SHAPE and raw_out(*po, Bm=2) == ERR_SHAPE, "Bm = 2 with B = 3"
    assert raw_in(*p, Cm=2) == ERR_SHAPE and raw_out(*po, Cm=3) == ERR_SHAPE
    for bad in (dict(B=0), dict(C=0), dict(HW=0), dict(HW=-35), dict(B=-3, Bm=-3)):
        assert raw_in(*p, **bad) == ERR_SHAPE and raw_out(*po, **bad) == ERR_SHAPE, bad
    big = dict(B=1 << 15, Bm=1, C=1 << 15, Cm=1, HW=2)                  # 2^31 floats: the kernels index in 32 bits
    assert raw_in(*p, **big) == ERR_SHAPE and raw_out(*po, **big) == ERR_SHAPE
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()), "a refused call launches nothing"
    with pytest.raises(ValueError, match="mask of shape"):
        ops.inpaint_in(dx, dm[:2].contiguous(), dl, dn, ds)
    with pytest.raises(ValueError, match="one device"):
        ops.inpaint_in(dx, dm.cpu(), dl, dn, ds)
    with pytest.raises(ValueError, match="sigma"):
        ops.inpaint_in(dx, dm, dl, dn, sigma)                           # sigma on the host
    with pytest.raises(ValueError, match="dtype"):
        ops.inpaint_out_(dx.half(), dm, dl)
    with pytest.raises(ValueError, match="contiguous"):
        ops.inpaint_out_(dx, dm, dl.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2))
    assert raw_in(*p) == OK and raw_out(*po) == OK
    torch.cuda.synchronize()
