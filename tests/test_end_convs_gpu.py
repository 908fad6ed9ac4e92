"""GPU: the 3- and 4-channel end convolutions of the upscaler and of the preview decoder alone (ld_op_esrgan_first / _last, ld_op_taesd_first /
_last: the launchers ld_esrgan_forward and ld_taesd_decode call), each held element-wise (tests/errbound.py) against the fp64 convolution of the
same inputs.  Inside the models a wrong tap on one border row moves the rel-L2 of the whole image by far less than its allowance; here every pixel
is held.  The batch case gives image 0's last row and image 1's first row large values, so a tap that walks from one image into its neighbour is
far outside the bound.  Each case prints its worst error / bound and signed bias.

KERNELS names, per kernel, the tests that hold it (tests/test_errbound_cpu.py keeps the ledger)."""
import math

import numpy as np
import pytest
import torch

import errbound as EB
import usdu_ref
from lightdiffusion_amd._lib import ERR_ARG, ERR_SHAPE

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

KERNELS = {
    "esrgan_first_kernel": ["test_esrgan_first", "test_end_conv_rejects"],
    "esrgan_last_kernel": ["test_esrgan_last", "test_end_conv_rejects"],
    "taesd_first_kernel": ["test_taesd_first", "test_end_conv_rejects"],
    "taesd_last_kernel": ["test_taesd_last", "test_end_conv_rejects"],
}
# under one block; one row; one column; a batch (an image's border reads zeros, not its neighbour); several blocks with a ragged last one
SIZES = [(1, 5, 7), (1, 1, 9), (1, 9, 1), (2, 9, 11), (1, 33, 47)]
SENTINEL = -21846          # 0xAAAA as int16: the bit pattern of the channels a kernel must not write


@pytest.fixture(scope="module")
def ops():
    from lightdiffusion_amd import ops as o
    from lightdiffusion_amd._lib import lib
    lib()
    return o


def held(y, ref, bound, what, h, w, keep=None):
    if keep is None:
        frac = EB.bias_kept_fraction(ref)
        assert frac >= 0.5, f"{what}: the bias statistic keeps only {frac:.2f} of the elements"
    r, s = EB.check(y, ref, bound, what, image_rows=h * w, width=w, keep=keep, bias_extra=EB.rtn_noise(EB.independent_roundings(ref, keep)))
    print(f"{what}: error / bound {r:.3f}, signed bias {s:+.2e}")
    return r, s


def inputs(n, h, w, cin, cout, seed, xscale=1.0, pitch=None):
    """x fp32 [n][h][w][pitch or cin] with, in a batch, image 0's last row and image 1's first row at 8x the size of the rest; weights for cin."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, h, w, pitch or cin, generator=g) * xscale
    if n > 1:
        x[0, h - 1] *= 8.0
        x[1, 0] *= 8.0
    wt = (torch.randn(cout, 9 * cin, generator=g) / math.sqrt(9 * cin)).half()
    b = (torch.randn(cout, generator=g) * 0.5).half()
    return x.to(DEV), wt.to(DEV), b.to(DEV), g


@pytest.mark.parametrize("n,h,w", SIZES)
def test_esrgan_first(ops, n, h, w):
    x, wt, b, _ = inputs(n, h, w, 3, 64, 100 * h + w)
    ref, bound = EB.esrgan_first_ref(x, wt, b)
    for ldy in (64, 192):
        for ldy2 in (None, 64, 192):
            y = torch.full((n, h, w, ldy), SENTINEL, dtype=torch.int16, device=DEV).view(torch.float16)
            y2 = None if ldy2 is None else torch.full((n, h, w, ldy2), SENTINEL, dtype=torch.int16, device=DEV).view(torch.float16)
            ops.esrgan_first(x, wt, b, y, y2)
            assert ops.last_kernel() == "esrgan_first_kernel"
            what = f"esrgan_first {n}x{h}x{w} ldy={ldy} ldy2={ldy2}"
            held(y[..., :64].reshape(-1, 64), ref, bound, what, h, w)
            assert bool((y[..., 64:].view(torch.int16) == SENTINEL).all()), f"{what}: channels behind 64 of y were written"
            if y2 is not None:
                assert torch.equal(y2[..., :64].view(torch.int16), y[..., :64].view(torch.int16)), f"{what}: the second copy differs"
                assert bool((y2[..., 64:].view(torch.int16) == SENTINEL).all()), f"{what}: channels behind 64 of y2 were written"


@pytest.mark.parametrize("n,h,w", SIZES)
def test_taesd_first(ops, n, h, w):
    """Latents up to |x| = 30 (tanh saturated: the operand is exactly +-3), exact zeros and negatives among them."""
    x, wt, b, g = inputs(n, h, w, 4, 64, 200 * h + w, xscale=2.5)
    x.clamp_(-30.0, 30.0)                                                  # (the batch case's two loud rows reach beyond)
    flat = x.view(-1)
    idx = torch.randperm(flat.numel(), generator=g)[:max(4, flat.numel() // 6)].to(DEV)
    vals = torch.tensor([30.0, -30.0, 0.0, -0.0, 12.0, -12.0], device=DEV)
    flat[idx] = vals[torch.arange(idx.numel(), device=DEV) % 6]
    assert float(x.abs().max()) == 30.0 and bool((x == 0).any()) and bool((x < 0).any())
    ref, bound = EB.taesd_first_ref(x, wt, b)
    y = ops.taesd_first(x, wt, b)
    assert ops.last_kernel() == "taesd_first_kernel"
    keep = ref > 0
    assert 0.2 < float(keep.double().mean()) < 0.8                        # both sides of the ReLU
    held(y.reshape(-1, 64), ref, bound, f"taesd_first {n}x{h}x{w}", h, w, keep=keep)
    assert float(y.min()) >= 0.0


@pytest.mark.parametrize("n,h,w", SIZES)
def test_esrgan_last(ops, n, h, w):
    for ldx in (64, 192):
        x, wt, b, _ = inputs(n, h, w, 64, 3, 300 * h + w + ldx, pitch=ldx)
        x = x.half()
        ref, bound = EB.esrgan_last_ref(x, wt, b)
        y = ops.esrgan_last(x, wt, b)
        assert ops.last_kernel() == "esrgan_last_kernel"
        held(y.reshape(-1, 3), ref, bound, f"esrgan_last {n}x{h}x{w} ldx={ldx}", h, w, keep=torch.ones_like(ref, dtype=torch.bool))


@pytest.mark.parametrize("n,h,w", SIZES)
def test_taesd_last(ops, n, h, w):
    """Weights and biases scaled so that d covers below -1, inside and above 1: both clip arms of the image.  The image: byte for byte
    to_u8((d + 1) * 0.5) of the DEVICE's own fp32 d (Pillow's truncation, tests/usdu_ref.py), and within one count of the fp64 reference's byte."""
    x, wt, _, _ = inputs(n, h, w, 64, 3, 400 * h + w)
    x = x.half()
    b = torch.tensor([0.5, -0.25, 1.5]).half().to(DEV)
    ref, bound, img_ref = EB.taesd_last_ref(x, wt, b)
    assert bool((ref < -1).any()) and bool((ref > 1).any()) and bool(((ref > -1) & (ref < 1)).any())
    d, img = ops.taesd_last(x, wt, b)
    assert ops.last_kernel() == "taesd_last_kernel"
    what = f"taesd_last {n}x{h}x{w}"
    held(d.reshape(-1, 3), ref, bound, what, h, w, keep=torch.ones_like(ref, dtype=torch.bool))
    got = img.cpu().numpy()
    want = usdu_ref.to_u8(((d.cpu() + 1.0) * 0.5).numpy())
    diff = np.argwhere(got != want)
    assert len(diff) == 0, f"{what}: {len(diff)} image bytes differ from to_u8 of the device's d, first at (image, row, column, channel) {tuple(diff[0])}"
    assert got.min() == 0 and got.max() == 255
    off = (torch.from_numpy(got.astype(np.int64)).reshape(-1, 3) - img_ref.cpu().long()).abs()
    assert int(off.max()) <= 1, f"{what}: image byte {int(off.max())} counts from the fp64 reference's at {EB.locate(int(off.flatten().argmax()), tuple(off.shape), h * w, w)}"
    d2, none = ops.taesd_last(x, wt, b, image=False)                      # without the image: the same d
    assert none is None and torch.equal(d2, d)


def test_end_conv_rejects(ops):
    """Refused on the host before any launch: the status, and ld_op_last_kernel() left as the previous call set it."""
    from lightdiffusion_amd._lib import lib
    l = lib()
    s = torch.cuda.current_stream().cuda_stream
    x3, wt3, b64, _ = inputs(1, 4, 4, 3, 64, 1)
    x4 = torch.zeros(1, 4, 4, 4, device=DEV)
    wt4 = torch.zeros(64, 36, dtype=torch.float16, device=DEV)
    x64, wtl, b3, _ = inputs(1, 4, 4, 64, 3, 2)
    x64 = x64.half()
    y = torch.zeros(1, 4, 4, 64, dtype=torch.float16, device=DEV)
    o = torch.zeros(1, 4, 4, 3, dtype=torch.float32, device=DEV)
    ops.taesd_first(x4, wt4, b64)
    before = ops.last_kernel()
    assert before == "taesd_first_kernel"
    p = lambda t: t.data_ptr()
    big = 1 << 30
    calls = [
        (ERR_ARG, lambda: l.ld_op_esrgan_first(None, p(wt3), p(b64), p(y), 64, None, 0, 1, 4, 4, s)),
        (ERR_ARG, lambda: l.ld_op_esrgan_first(p(x3), None, p(b64), p(y), 64, None, 0, 1, 4, 4, s)),
        (ERR_ARG, lambda: l.ld_op_esrgan_first(p(x3), p(wt3), None, p(y), 64, None, 0, 1, 4, 4, s)),
        (ERR_ARG, lambda: l.ld_op_esrgan_first(p(x3), p(wt3), p(b64), None, 64, None, 0, 1, 4, 4, s)),
        (ERR_SHAPE, lambda: l.ld_op_esrgan_first(p(x3), p(wt3), p(b64), p(y), 56, None, 0, 1, 4, 4, s)),          # a pitch below the 64 channels written
        (ERR_SHAPE, lambda: l.ld_op_esrgan_first(p(x3), p(wt3), p(b64), p(y), 68, None, 0, 1, 4, 4, s)),          # not a multiple of 8
        (ERR_SHAPE, lambda: l.ld_op_esrgan_first(p(x3), p(wt3), p(b64), p(y), 64, p(y), 60, 1, 4, 4, s)),
        (ERR_SHAPE, lambda: l.ld_op_esrgan_first(p(x3), p(wt3), p(b64), p(y), 64, None, 0, 0, 4, 4, s)),
        (ERR_SHAPE, lambda: l.ld_op_esrgan_first(p(x3), p(wt3), p(b64), p(y), 64, None, 0, 1, -1, 4, s)),
        (ERR_SHAPE, lambda: l.ld_op_esrgan_first(p(x3), p(wt3), p(b64), p(y), 64, None, 0, 1, 4, 0, s)),
        (ERR_SHAPE, lambda: l.ld_op_esrgan_first(p(x3), p(wt3), p(b64), p(y), 64, None, 0, 64, big, 64, s)),      # 2^42 pixels: no grid holds them
        (ERR_ARG, lambda: l.ld_op_esrgan_last(None, 64, p(wtl), p(b3), p(o), 1, 4, 4, s)),
        (ERR_ARG, lambda: l.ld_op_esrgan_last(p(x64), 64, p(wtl), p(b3), None, 1, 4, 4, s)),
        (ERR_SHAPE, lambda: l.ld_op_esrgan_last(p(x64), 32, p(wtl), p(b3), p(o), 1, 4, 4, s)),
        (ERR_SHAPE, lambda: l.ld_op_esrgan_last(p(x64), 100, p(wtl), p(b3), p(o), 1, 4, 4, s)),
        (ERR_SHAPE, lambda: l.ld_op_esrgan_last(p(x64), 64, p(wtl), p(b3), p(o), 1, 0, 4, s)),
        (ERR_SHAPE, lambda: l.ld_op_esrgan_last(p(x64), 64, p(wtl), p(b3), p(o), big, big, 2, s)),
        (ERR_ARG, lambda: l.ld_op_taesd_first(None, p(wt4), p(b64), p(y), 1, 4, 4, s)),
        (ERR_ARG, lambda: l.ld_op_taesd_first(p(x4), p(wt4), None, p(y), 1, 4, 4, s)),
        (ERR_SHAPE, lambda: l.ld_op_taesd_first(p(x4), p(wt4), p(b64), p(y), 1, 4, -3, s)),
        (ERR_SHAPE, lambda: l.ld_op_taesd_first(p(x4), p(wt4), p(b64), p(y), 1 << 20, 1 << 20, 1, s)),
        (ERR_SHAPE, lambda: l.ld_op_taesd_first(p(x4), p(wt4), p(b64), p(y), 1, 1 << 20, 1 << 20, s)),           # n h fits, the pixels do not
        (ERR_ARG, lambda: l.ld_op_taesd_last(p(x64), None, p(b3), p(o), None, 1, 4, 4, s)),
        (ERR_ARG, lambda: l.ld_op_taesd_last(p(x64), p(wtl), p(b3), None, None, 1, 4, 4, s)),
        (ERR_SHAPE, lambda: l.ld_op_taesd_last(p(x64), p(wtl), p(b3), p(o), None, 0, 4, 4, s)),
        (ERR_SHAPE, lambda: l.ld_op_taesd_last(p(x64), p(wtl), p(b3), p(o), None, big, big, big, s)),
    ]
    for k, (want, call) in enumerate(calls):
        assert call() == want, f"rejection {k}"
        assert ops.last_kernel() == before, f"rejection {k} changed ld_op_last_kernel()"
    torch.cuda.synchronize()
    assert bool((y == 0).all()) and bool((o == 0).all())                  # and nothing was written
