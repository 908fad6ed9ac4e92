"""GPU: the Detailer's three fp32 image kernels (csrc/detail/detail_image.hip) through lightdiffusion_amd.ops, on the op cases of
tests/detailer_standins.py and, beyond one lap of their grid-stride loops, on one larger case each.
  crop   bitwise against detailer_ref.crop_u8 and against tensor2pil's expression in torch (what test_detailer_cpu.py holds the reference to)
  blur   within detailer_ref.blur_bound of the fp64 blur, within the recorded restatement's own error plus that bound of the golden, and BITWISE
         against the kernel's order of operations written out in torch fp32 (test_detail_ops_cpu.blur_restated, held to the bound on the CPU)
  paste  bitwise against detailer_ref.paste and against tensor_paste in torch; every float outside the clipped window untouched
(tests/golden/detailer_ops.npz records blur outputs only; crop and paste are exact, so their second reference is the torch expression.)
KERNELS names the tests that hold each kernel; tests/test_detail_ledger_cpu.py keeps that ledger."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detailer_ref as R                                              # noqa: E402
import detailer_standins as S                                         # noqa: E402
from test_detail_ops_cpu import LAP_BLUR, bits, blur_restated, lap_mask      # noqa: E402
from test_detailer_cpu import GOLDEN, torch_paste                     # noqa: E402
from lightdiffusion_amd import ops                                    # noqa: E402
from lightdiffusion_amd._lib import ERR_ARG, ERR_SHAPE, OK, lib       # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAP = 4096 * 256                    # work items in one lap of a grid-stride loop: 4096 blocks of 256 lanes

KERNELS = {
    "crop_u8_kernel": ("test_crop", "test_crop_beyond_one_lap_and_on_the_vector_paths"),
    "gauss_axis_kernel": ("test_blur", "test_blur_beyond_one_lap", "test_blur_of_a_pitched_window"),
    "paste_u8_kernel": ("test_paste", "test_paste_beyond_one_lap", "test_paste_alpha_of_zero_and_one"),
}


@pytest.fixture(scope="module")
def ops_golden():
    return np.load(os.path.join(GOLDEN, "detailer_ops.npz"))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def tensor2pil_u8(canvas, x1, y1, x2, y2):
    """np.clip(255. * tensor, 0, 255).astype(uint8) of the window, through torch as the reference takes it"""
    return np.clip(255.0 * torch.from_numpy(canvas)[None, y1:y2, x1:x2].numpy().squeeze(0), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------ crop
@pytest.mark.parametrize("win", S.CROP_WINDOWS)
def test_crop(win):
    canvas = S.crop_canvas()
    d = dev(canvas)
    got = ops.u8_crop_from_f32(d, *win)
    want = R.crop_u8(canvas, *win)
    assert got.dtype == torch.uint8 and got.is_contiguous() and tuple(got.shape) == want.shape
    assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(want, tensor2pil_u8(canvas, *win))
    assert np.array_equal(bits(d.cpu().numpy()), bits(canvas)), "the canvas is read only"
    if win == (0, 0, 53, 37):                      # every special value of the canvas is inside: k / 255 +- 1 ulp, below 0, above 1, -0.0
        assert want.min() == 0 and want.max() == 255 and np.signbit(canvas[canvas == 0.0]).any()


def test_crop_beyond_one_lap_and_on_the_vector_paths():
    """1208 x 1200: a row pitch of 3624 floats, so a window at x1 = 4 has 16-byte aligned rows of 3600 floats — vector loads and word stores, and
    900 x 1200 work items is more than one lap; at x1 = 5 the same rows are unaligned (scalar loads), 3597 floats wide (byte stores, a tail);
    the whole canvas is dense on both sides and runs as one flat row."""
    rng = np.random.default_rng(11)
    canvas = rng.random((1200, 1208, 3), dtype=np.float32) * np.float32(1.4) - np.float32(0.2)
    d = dev(canvas)
    assert 1200 * (3600 // 4) > LAP
    for win in [(4, 0, 1204, 1200), (5, 0, 1204, 1200), (0, 0, 1208, 1200), (8, 3, 12, 1199)]:
        assert np.array_equal(ops.u8_crop_from_f32(d, *win).cpu().numpy(), R.crop_u8(canvas, *win)), win
    assert np.array_equal(bits(d.cpu().numpy()), bits(canvas))


def test_crop_rejections():
    d = dev(S.crop_canvas())
    for win in [(-1, 0, 5, 5), (0, 0, 54, 5), (0, 0, 5, 38), (5, 5, 5, 9), (9, 5, 5, 9)]:
        with pytest.raises(ValueError, match="window"):
            ops.u8_crop_from_f32(d, *win)
    with pytest.raises(ValueError, match="device"):
        ops.u8_crop_from_f32(d.cpu(), 0, 0, 5, 5)
    with pytest.raises(ValueError, match="dtype"):
        ops.u8_crop_from_f32(d.half(), 0, 0, 5, 5)
    out = torch.zeros(5, 5, 3, dtype=torch.uint8, device=DEV)
    raw = lambda *a: lib().ld_op_f32_crop_u8(d.data_ptr(), 159, 53, 37, 3, *a, out.data_ptr(), 15, None)
    assert raw(0, 0, 54, 5) == ERR_ARG and raw(0, 0, 5, 38) == ERR_ARG and raw(-1, 0, 4, 5) == ERR_ARG
    assert lib().ld_op_f32_crop_u8(d.data_ptr(), 158, 53, 37, 3, 0, 0, 5, 5, out.data_ptr(), 15, None) == ERR_SHAPE
    assert lib().ld_op_f32_crop_u8(d.data_ptr(), 159, 53, 37, 3, 0, 0, 5, 5, out.data_ptr(), 14, None) == ERR_SHAPE
    torch.cuda.synchronize()
    assert int(out.sum()) == 0, "a refused call launches nothing"


# ------------------------------------------------------------------ blur
@pytest.mark.parametrize("h,w,feather", S.BLUR_CASES)
def test_blur(ops_golden, h, w, feather):
    mask = S.blur_mask(h, w, feather)
    d = dev(mask)
    got = ops.f32_gaussian_blur(d, feather)
    again = ops.f32_gaussian_blur(d, feather, 10.0)
    assert got.dtype == torch.float32 and got.is_contiguous() and tuple(got.shape) == (h, w) and got.data_ptr() != d.data_ptr()
    got, again = got.cpu().numpy(), again.cpu().numpy()
    name = S.blur_name(h, w, feather)
    err = float(np.abs(got.astype(np.float64) - R.gaussian_blur(mask, feather)).max())
    gold = float(np.abs(got.astype(np.float64) - ops_golden["blur_" + name].astype(np.float64)).max())
    print(f"blur {name}: vs fp64 {err:.3e} (bound {R.blur_bound(feather):.3e}), vs the recorded restatement {gold:.3e}")
    assert err <= R.blur_bound(feather)
    assert gold <= float(ops_golden["blur_" + name + "_ref_err"]) + R.blur_bound(feather)
    assert np.array_equal(bits(got), bits(again)), "two runs give the same bits"
    assert np.array_equal(bits(got), bits(blur_restated(mask, feather))), "the kernel's order of operations is the restatement's"
    assert np.array_equal(bits(d.cpu().numpy()), bits(mask)), "the mask is read only"
    if feather == 0:
        assert np.array_equal(bits(got), bits(mask)), "feather 0 is a copy"


def test_blur_beyond_one_lap():
    h, w, feather = LAP_BLUR
    assert h * w > LAP
    mask = lap_mask()
    got = ops.f32_gaussian_blur(dev(mask), feather).cpu().numpy()
    err = float(np.abs(got.astype(np.float64) - R.gaussian_blur(mask, feather)).max())
    print(f"blur {h}x{w}_f{feather}: vs fp64 {err:.3e} (bound {R.blur_bound(feather):.3e})")
    assert err <= R.blur_bound(feather)
    assert np.array_equal(bits(got), bits(blur_restated(mask, feather)))


def test_blur_of_a_pitched_window():
    """A view of a larger mask (pointer + pitch) gives the bits of the dense copy, and reads nothing of what surrounds it: the surroundings are
    NaN, which any tap would carry into the result."""
    h, w, feather = 40, 56, 5
    mask = S.blur_mask(h, w, feather)
    big = np.full((h + 9, w + 13), np.nan, np.float32)
    big[4:4 + h, 7:7 + w] = mask
    d = dev(big)
    got = ops.f32_gaussian_blur(d[4:4 + h, 7:7 + w], feather).cpu().numpy()
    dense = ops.f32_gaussian_blur(dev(mask), feather).cpu().numpy()
    assert np.isfinite(got).all() and np.array_equal(bits(got), bits(dense))
    zero = ops.f32_gaussian_blur(d[4:4 + h, 7:7 + w], 0).cpu().numpy()       # the copy takes the pitch too
    assert np.array_equal(bits(zero), bits(mask))


def test_blur_rejections():
    limit = ops.f32_blur_max_feather()
    assert limit >= 100
    d = dev(S.blur_mask(6, 9, 5))
    for feather in (6, 7, 9, -1):
        with pytest.raises(ValueError, match="feather"):
            ops.f32_gaussian_blur(d, feather)
    ops.f32_gaussian_blur(d, 5)
    big = torch.zeros(limit + 2, limit + 2, device=DEV)
    ops.f32_gaussian_blur(big, limit)
    with pytest.raises(ValueError, match="limit"):
        ops.f32_gaussian_blur(torch.zeros(limit + 3, limit + 3, device=DEV), limit + 1)
    with pytest.raises(ValueError, match="device"):
        ops.f32_gaussian_blur(d.cpu(), 2)
    with pytest.raises(ValueError, match="dtype"):
        ops.f32_gaussian_blur(d.double(), 2)
    with pytest.raises(ValueError, match="shape"):
        ops.f32_gaussian_blur(d[None], 2)
    # the raw entry: LD_ERR_SHAPE and no launch — the destination keeps its sentinel
    out = torch.full((6, 9), -7.0, device=DEV)
    taps = ops.gaussian_taps(6).to(DEV)
    tmp = torch.empty(lib().ld_op_f32_blur_tmp_bytes(9, 6), dtype=torch.uint8, device=DEV)
    assert lib().ld_op_f32_blur_tmp_bytes(9, 6) >= 6 * 9 * 4
    raw = lambda feather: lib().ld_op_f32_gaussian_blur(d.data_ptr(), 9, out.data_ptr(), 9, 9, 6, feather, taps.data_ptr(), tmp.data_ptr(), None)
    assert raw(6) == ERR_SHAPE and raw(9) == ERR_SHAPE and raw(limit + 1) == ERR_SHAPE and raw(-1) == ERR_ARG
    assert lib().ld_op_f32_gaussian_blur(d.data_ptr(), 8, out.data_ptr(), 9, 9, 6, 2, taps.data_ptr(), tmp.data_ptr(), None) == ERR_SHAPE
    assert lib().ld_op_f32_gaussian_blur(d.data_ptr(), 9, out.data_ptr(), 9, 9, 6, 2, None, tmp.data_ptr(), None) == ERR_ARG
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()), "a refused call launches nothing"
    assert raw(0) == OK                                                       # feather 0 needs neither taps nor a temporary
    torch.cuda.synchronize()
    assert torch.equal(out, d)


# ------------------------------------------------------------------ paste
def check_paste(canvas, tile, alpha, x0, y0):
    d = dev(canvas)
    got = ops.f32_paste_u8_(d, dev(tile), dev(alpha), x0, y0)
    assert got is d
    got = got.cpu().numpy()
    want = R.paste(canvas.copy(), tile, alpha, x0, y0)
    assert np.array_equal(bits(got), bits(want))
    h, w = min(canvas.shape[0], y0 + tile.shape[0]) - y0, min(canvas.shape[1], x0 + tile.shape[1]) - x0
    outside = np.ones(canvas.shape[:2], bool)
    outside[y0:y0 + h, x0:x0 + w] = False
    assert np.array_equal(bits(got[outside]), bits(canvas[outside])), "floats outside the clipped window are untouched"
    assert not np.array_equal(bits(got[~outside]), bits(canvas[~outside]))
    return got


@pytest.mark.parametrize("name", list(S.PASTE_CASES))
def test_paste(name):
    x0, y0, _ = S.PASTE_CASES[name]
    tile, alpha = S.paste_inputs(name)
    got = check_paste(S.paste_canvas(), tile, alpha, x0, y0)
    assert np.array_equal(bits(got), bits(torch_paste(S.paste_canvas(), tile, alpha, x0, y0)))       # tensor_paste as the reference writes it
    if name == "clipped":
        assert x0 + tile.shape[1] > 53 and y0 + tile.shape[0] > 37


def test_paste_beyond_one_lap():
    """600 x 600 x 3 floats is more than one lap; the tile and the alpha are views (pitched) and the tile hangs over the canvas's corner."""
    rng = np.random.default_rng(13)
    canvas = rng.random((700, 640, 3), dtype=np.float32)
    tile = rng.integers(0, 256, (620, 620, 3), dtype=np.uint8)
    alpha = rng.random((620, 620), dtype=np.float32)
    assert 600 * 600 * 3 > LAP
    check_paste(canvas, tile, alpha, 40, 100)                                     # clipped to 600 x 600
    d, t, a = dev(canvas), dev(tile), dev(alpha)
    ops.f32_paste_u8_(d[10:690, 5:635], t[3:603, 9:609], a[1:601, 2:602], 7, 11)    # a window of the canvas, of the tile and of the alpha
    want = canvas.copy()
    R.paste(want[10:690, 5:635], tile[3:603, 9:609], alpha[1:601, 2:602], 7, 11)
    assert np.array_equal(bits(d.cpu().numpy()), bits(want))


@pytest.mark.parametrize("name", list(S.PASTE_CASES))
def test_paste_alpha_of_zero_and_one(name):
    x0, y0, _ = S.PASTE_CASES[name]
    tile, alpha = S.paste_inputs(name)
    canvas = S.paste_canvas()
    zero = ops.f32_paste_u8_(dev(canvas), dev(tile), dev(np.zeros_like(alpha)), x0, y0).cpu().numpy()
    assert np.array_equal(bits(zero), bits(canvas)), "alpha 0 leaves the canvas's bits"
    one = ops.f32_paste_u8_(dev(canvas), dev(tile), dev(np.ones_like(alpha)), x0, y0).cpu().numpy()
    h, w = min(37, y0 + tile.shape[0]) - y0, min(53, x0 + tile.shape[1]) - x0
    assert np.array_equal(bits(one[y0:y0 + h, x0:x0 + w]), bits(R.to_f32(tile[:h, :w]))), "alpha 1 gives tile / 255"
    mixed = alpha.copy()
    mixed[::2] = 0.0
    mixed[1::4] = 1.0
    check_paste(canvas, tile, mixed, x0, y0)


def test_paste_rejections():
    canvas, (tile, alpha) = dev(S.paste_canvas()), map(dev, S.paste_inputs("inside"))
    before = canvas.clone()
    with pytest.raises(ValueError, match="alpha of shape"):
        ops.f32_paste_u8_(canvas, tile, alpha[:, :-1], 5, 7)
    with pytest.raises(ValueError, match="origin"):
        ops.f32_paste_u8_(canvas, tile, alpha, 53, 0)
    with pytest.raises(ValueError, match="origin"):
        ops.f32_paste_u8_(canvas, tile, alpha, 0, -1)
    with pytest.raises(ValueError, match="device"):
        ops.f32_paste_u8_(canvas, tile.cpu(), alpha, 5, 7)
    with pytest.raises(ValueError, match="dtype"):
        ops.f32_paste_u8_(canvas, tile.float(), alpha, 5, 7)
    with pytest.raises(ValueError, match="dtype"):
        ops.f32_paste_u8_(canvas, tile, alpha.double(), 5, 7)
    with pytest.raises(ValueError, match="channels"):
        ops.f32_paste_u8_(canvas, tile[:, :, :2], alpha, 5, 7)
    raw = lambda x0, y0, tp=93: lib().ld_op_f32_paste_u8(canvas.data_ptr(), 159, 53, 37, 3, tile.data_ptr(), tp, alpha.data_ptr(), 31, 31, 20, x0, y0, None)
    assert raw(53, 0) == ERR_ARG and raw(0, 37) == ERR_ARG and raw(-1, 0) == ERR_ARG and raw(5, 7, 92) == ERR_SHAPE
    torch.cuda.synchronize()
    assert torch.equal(canvas, before), "a refused call launches nothing"
