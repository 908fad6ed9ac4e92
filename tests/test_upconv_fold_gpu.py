"""The UNet's Upsample1 layers on the folded weights (upconv route): nearest-2x + 3x3 convolution as four 2x2 convolutions of the source.

Route names, an element-wise bound against the UN-folded fp64 convolution, exact borders, re-derivation after a parameter load, the
fallbacks, and completeness against the profiled forwards.

Bound (derived, tests/errbound.py): the reference is the fp64 3x3 convolution of the nearest-upsampled fp16 input with the ORIGINAL fp16
weights.  The kernel multiplies the source pixels with the phase-tap weights w' (sums of 1, 2 or 4 taps, fp32 sum rounded to fp16 once) in
an fp32 MFMA chain of length 4 Cin and rounds the output once:
    |y - y_hat| <= 2^-11 |y_hat| + c_acc(4 Cin) sum |w' x| + 2^-11 sum_{summed w'} |w' x| + (bias add, staging: errbound.epilogue_ref) + 2^-24
The fold's term runs over the 12 summed phase-taps only: a single tap is copied, not rounded.  Signed bias as every route row: 2^-11 / 8.
"""
import ctypes as C
import math

import pytest
import torch

import errbound as EB
import upconv_ref as UR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAME = "upconv_kernel<256,320>"
NAME_SPLIT = NAME + "+upconv_reduce_kernel"
PINNED = {NAME, NAME_SPLIT}


@pytest.fixture(scope="module")
def ops():
    from lightdiffusion_amd import ops as o
    from lightdiffusion_amd._lib import lib
    lib()
    return o


def r16(shape, seed, scale=1.0, offset=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale + offset).half().to(DEV)


# (n, h, w, c, expected route): the three Upsample1 layers of the SD1.5 UNet at n = 16 (batch 8, CFG pair) and n = 3 (the smallest batch
# above the row-resident kernel's).  Tiles of 256 source pixels x 320 of the 4 c columns; fewer than 192 of them split over K (<= K / 640 slices).
UP_ROUTES = [
    (16, 32, 32, 640, NAME),           # 64 x 8 tiles
    (16, 16, 16, 1280, NAME),          # 16 x 16 tiles
    (16, 8, 8, 1280, NAME_SPLIT),      # 4 x 16 tiles, 4 slices
    (3, 32, 32, 640, NAME_SPLIT),      # 12 x 8 tiles, 3 slices
    (3, 16, 16, 1280, NAME_SPLIT),     # 3 x 16 tiles, 6 slices
    (3, 8, 8, 1280, NAME_SPLIT),       # one ragged row of 16 tiles, 8 slices
]


def fold_ref(x, wt, b):
    """y_hat [n][2h][2w][O] (un-folded fp64 convolution) and its bound (module docstring)."""
    n, h, w, c = x.shape
    O = wt.shape[0]
    ref, _, _ = EB.conv_ref(x, wt, None, out_hw=(2 * h, 2 * w))
    ref = ref.reshape(n, 2 * h, 2 * w, O)
    wf = UR.fold_weights(wt.double())
    xd = x.double()
    absdot, foldabs, same = {}, {}, {}
    for py in (0, 1):
        for px in (0, 1):
            A, Wm = UR.phase_operands(xd, wf, py, px)
            absdot[(py, px)] = A.abs() @ Wm.abs().t()
            same[(py, px)] = A @ Wm.t()
            As, Ws = UR.phase_operands(xd, wf, py, px, only_sums=True)
            foldabs[(py, px)] = As.abs() @ Ws.abs().t()
    # the fold is exact algebra: both fp64 evaluations agree far below the bound
    assert torch.allclose(UR.interleave(same, n, h, w), ref, rtol=1e-9, atol=1e-9)
    y, bound = EB.epilogue_ref(ref, UR.interleave(absdot, n, h, w), 4 * c, b, None, extra=EB.U * UR.interleave(foldabs, n, h, w))
    return y, bound


@pytest.mark.parametrize("n,h,w,c,route", UP_ROUTES, ids=lambda v: str(v))
def test_upconv_route(ops, n, h, w, c, route):
    x = r16((n, h, w, c), 71)
    wt = r16((c, c, 3, 3), 72, 1 / math.sqrt(9 * c))
    b = r16((c,), 73, 0.5)
    wp = ops.repack_conv_weight(wt)
    y = ops.upconv2x(x, wp, ops.upconv2x_fold(wp), b)
    assert ops.last_kernel() == route
    ref, bound = fold_ref(x, wt, b)
    r, s = EB.check(y.reshape(-1, c), ref.reshape(-1, c), bound.reshape(-1, c), f"{route} n{n} {h}x{w} c{c}", image_rows=4 * h * w, width=2 * w)
    print(f"{route} n{n} {h}x{w} c{c}: worst error / bound {r:.3f}, signed bias {s:.3g}")


def test_fold_weights_are_the_rounded_sums(ops):
    """The device fold against the fp64 table: single taps copied exactly, sums within half an ulp of the exact sum."""
    c, o = 64, 320
    wt = r16((o, c, 3, 3), 74, 1 / math.sqrt(9 * c))
    wf = ops.upconv2x_fold(ops.repack_conv_weight(wt)).reshape(2, 2, o, 2, 2, c)        # [py][px][O][a][b][I]
    want = UR.fold_weights(wt.double()).permute(0, 1, 4, 2, 3, 5)                      # -> the same order
    assert torch.equal(wf.double(), want.half().double())                              # (fp32 sums of <= 4 fp16 values are exact: one rounding)


@pytest.mark.parametrize("n,h,w,c", [(3, 32, 32, 640), (3, 16, 16, 1280), (3, 8, 8, 1280), (16, 16, 16, 1280)], ids=lambda v: str(v))
def test_borders_are_exact(ops, n, h, w, c):
    """Ones in, ones as weights: an output pixel counts the taps inside the upsampled image — 4 c at the corners, 6 c on the edges, 9 c
    inside, all exactly representable.  A wrong phase table or zero-page case shows here as a wrong integer at a named place."""
    x = torch.ones(n, h, w, c, dtype=torch.float16, device=DEV)
    wp = ops.repack_conv_weight(torch.ones(c, c, 3, 3, dtype=torch.float16, device=DEV))
    y = ops.upconv2x(x, wp, ops.upconv2x_fold(wp), None).float()
    assert ops.last_kernel() in PINNED
    cy = torch.full((2 * h,), 3.0, device=DEV)
    cy[0] = cy[-1] = 2.0
    cx = torch.full((2 * w,), 3.0, device=DEV)
    cx[0] = cx[-1] = 2.0
    want = (cy[:, None] * cx[None, :] * c).view(1, 2 * h, 2 * w, 1).expand_as(y)
    bad = (y != want).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} wrong elements, first (image, row, column, channel) {bad[0].tolist()}: got {float(y[tuple(bad[0])])}, want {float(want[tuple(bad[0])])}"


def test_fallbacks_keep_their_routes(ops):
    """Offered folded weights change nothing where the planner declines them: a resize that is not 2x, and a two-image batch (the
    row-resident kernel's) dispatch what ld_op_conv dispatches, with the same bits."""
    for n, h, w, c, cout, out_hw, route in [
        (2, 8, 8, 320, 320, (11, 9), "gemm3_kernel<64,160,conv,deep>+splitk_reduce_kernel"),
        (12, 8, 8, 320, 320, (17, 16), None),
        (2, 8, 8, 640, 640, (16, 16), "conv8_kernel<W16,up>"),
        (2, 16, 16, 320, 320, (32, 32), "conv8_kernel<W32,up>"),
        (2, 32, 32, 640, 640, (64, 64), None),             # two images that the row-resident kernel does not take either
    ]:
        x = r16((n, h, w, c), 75)
        wt = r16((cout, c, 3, 3), 76, 1 / math.sqrt(9 * c))
        b = r16((cout,), 77, 0.5)
        wp = ops.repack_conv_weight(wt)
        want = ops.conv2d(x, wp, b, out_hw=out_hw)
        today = ops.last_kernel()
        got = ops.upconv2x(x, wp, ops.upconv2x_fold(wp), b, out_hw=out_hw)
        assert ops.last_kernel() == today and not today.startswith("upconv")
        if route is not None:
            assert today == route
        assert torch.equal(got, want)


def _small_cfg():
    # two levels of 320 channels: one Upsample1 (output_blocks.1.1), 320 -> 320 at 8x8 -> 16x16, one transformer per level-0 output block
    return dict(in_channels=4, out_channels=4, model_channels=320, channel_mult=[1, 1], num_res_blocks=[1, 1], transformer_depth=[1, 0],
                transformer_depth_output=[1, 1, 0, 0], transformer_depth_middle=0, context_dim=64, num_heads=8)


def test_fold_is_rederived_after_load_param():
    """ld_unet_load_param after a forward: the next forward runs on phase weights derived from the NEW 3x3 weights — bit-identical to an
    executor that was built with them."""
    from lightdiffusion_amd import weights as W
    from lightdiffusion_amd._lib import F16, check, lib
    from lightdiffusion_amd.unet import MI355XUNet
    cfg = _small_cfg()
    key = "output_blocks.1.1.conv.weight"
    sd = W.synth_state_dict(W.unet_param_shapes(cfg))
    assert key in sd
    new_w = (torch.randn(sd[key].shape, generator=torch.Generator().manual_seed(5)) * 0.02).half()
    n = 4
    x = torch.randn(n, 4, 16, 16, generator=torch.Generator().manual_seed(6)).to(DEV)
    sigma = torch.full((n,), 2.0, device=DEV)
    ctx = torch.randn(n, 77, 64, generator=torch.Generator().manual_seed(7))
    a = MI355XUNet(cfg, sd, max_batch=n, max_hw=(16, 16))
    a.set_context(ctx)
    a.profile(x, sigma)
    assert sum(k.startswith(NAME) for k in a.profile_kernels()) == 1, "the small UNet's Upsample1 does not run the folded route"
    y0 = a.forward(x, sigma).clone()
    t = new_w.to(DEV).contiguous()
    check(lib().ld_unet_load_param(a._h, key.encode(), t.data_ptr(), F16, torch.cuda.current_stream().cuda_stream), "load_param")
    y1 = a.forward(x, sigma).clone()
    sd2 = dict(sd)
    sd2[key] = new_w
    b = MI355XUNet(cfg, sd2, max_batch=n, max_hw=(16, 16))
    b.set_context(ctx)
    y2 = b.forward(x, sigma)
    assert not torch.equal(y0, y1), "the forward ignored the loaded parameter"
    assert torch.equal(y1, y2), f"stale folded weights: max |diff| {float((y1 - y2).abs().max())}"


@pytest.mark.parametrize("batch,hw,count", [(8, 64, 3), (4, 128, 3), (1, 64, 0)])
def test_unet_forward_dispatches_the_folded_route(batch, hw, count):
    """The profiled SD1.5 forward (CFG pair): three Upsample1 launches on the folded route at batch 8 and at the hires step, none at
    batch 1; every name of the family is pinned above; the launches stay in class conv3 and are counted as the 3x3 convolution they
    implement (2 (4 M) Cout 9 Cin FLOPs: last_flops is algorithmic work, the kernel executes 4/9 of it)."""
    from lightdiffusion_amd import weights as W
    from lightdiffusion_amd.unet import synthetic_unet
    u = synthetic_unet(W.sd15_unet_config(), max_batch=2 * batch, max_hw=(hw, hw))
    u.set_context(torch.randn(2 * batch, 77, 768))
    u.profile_pair(torch.randn(batch, 4, hw, hw, device=DEV), torch.full((batch,), 3.0, device=DEV))
    rows = [r for r in u.profile_launches() if r[-1].startswith("upconv")]
    assert {r[-1] for r in rows} <= PINNED, sorted({r[-1] for r in rows} - PINNED)
    assert len(rows) == count
    for what, (M, N, K, _), fl, us, kern in rows:
        assert what == "conv3" and K == 9 * N and fl == 2.0 * M * N * K
        print(f"b{batch} {hw}^2: {M} x {N} x {K}  {us:.1f} us  {kern}")
    if count == 0:
        assert any(r[-1].startswith("conv8_kernel<W16,up>") for r in u.profile_launches())
