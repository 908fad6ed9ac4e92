"""GPU: UltimateSDUpscale on the device.  The 8-bit image kernels (image.hip) against Pillow's recorded outputs (tests/golden/usdu_ops.npz) and,
beyond one lap of their grid-stride loops, on two and four channels, on every alignment path and with a blur radius beyond the image, against the
NumPy restatement of Pillow's arithmetic (tests/usdu_ref.py, which tests/test_usdu_cpu.py holds to Pillow itself): 0 differing bytes; KERNELS names
the tests that hold each kernel (tests/test_errbound_cpu.py keeps the ledger); the node with the stand-in stages against the reference's recorded run (usdu_flow.npz): every canvas byte for byte; the
node with the real stages against the same job loop written here from usdu_ref and the package's existing nodes: identical bytes; and a
full-size run (544 x 544 redraw tiles) on SD1.5-sized synthetic weights."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import usdu_ref as R            # noqa: E402
import usdu_standins as S       # noqa: E402
from test_usdu_cpu import GOLDEN, ref_resample, run_flow      # noqa: E402
from lightdiffusion_amd import nodes as N                     # noqa: E402
from lightdiffusion_amd import ops, usdu                      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOKS = [[(49406, 1.0)] + [(320, 1.0)] * 3 + [(49407, 1.0)] * 73]


@pytest.fixture(scope="module")
def ops_golden():
    return np.load(os.path.join(GOLDEN, "usdu_ops.npz"))


@pytest.fixture(scope="module")
def flow_golden():
    return np.load(os.path.join(GOLDEN, "usdu_flow.npz"))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same(got, want, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    n = int((got != want).sum())
    assert n == 0, f"{what}: {n} differing bytes"


# ------------------------------------------------------------------ the ops
@pytest.mark.parametrize("name", list(S.resample_cases()))
def test_resample(ops_golden, name):
    src, box, size, filt = S.resample_cases()[name]
    img = dev(src)
    view = img if box is None else img[box[1]:box[3], box[0]:box[2]]          # a window of the larger image: pointer + pitch, no copy
    same(ops.u8_resample(view, size, filt), ops_golden["resample_" + name], name)
    if box is not None:
        same(img, src, "the source around the window")


@pytest.mark.parametrize("name", list(S.blur_cases()))
def test_blur(ops_golden, name):
    mask, radius = S.blur_cases()[name]
    same(ops.u8_gaussian_blur(dev(mask), radius), ops_golden["blur_" + name], name)


def test_blur_weights_and_window(ops_golden):
    for r in (2.5, 4, 8, 16):
        assert ops.u8_box_weights(r) == R.box_weights(r), r
    assert ops.u8_box_weights(16)[0] == 15 and ops.u8_blur_reach(16) == 48
    mask, radius = S.blur_cases()["r2p5"]                                      # 50 x 70, reach 9
    full = ops_golden["blur_r2p5"]
    for region in [(20, 15, 41, 30), (0, 0, 12, 50), (55, 38, 70, 50)]:         # interior; flush with the left edge; the far corner
        got = ops.u8_gaussian_blur(dev(mask), radius, region)
        same(got, full[region[1]:region[3], region[0]:region[2]], f"window {region}")
    # the mask of one job, built in the window and blurred there, against the full-canvas mask
    rect, region = (64, 32, 33, 33), (50, 20, 80, 70)                           # hangs over the right edge of an 80-wide canvas
    want = np.zeros((96, 80), np.uint8)
    want[32:65, 64:80] = 255
    same(ops.u8_region_mask((96, 80), rect, None, 4, region, DEV), R.gaussian_blur(want, 4)[20:70, 50:80], "region mask")
    same(ops.u8_region_mask((96, 80), rect, None, 0, region, DEV), want[20:70, 50:80], "region mask without blur")


@pytest.mark.parametrize("name", list(S.composite_cases()))
def test_composite(ops_golden, name):
    canvas, tile, alpha, x0, y0 = S.composite_cases()[name]
    got = ops.u8_composite_(dev(canvas), dev(tile), dev(alpha), x0, y0)
    want = ops_golden["composite_" + name]
    same(got, want, name)
    outside = np.ones(canvas.shape[:2], bool)
    outside[y0:y0 + alpha.shape[0], x0:x0 + alpha.shape[1]] = False
    assert np.array_equal(got.cpu().numpy()[outside], canvas[outside])          # bytes outside the region unchanged
    if name == "inner":                                                          # alpha rows of 0 and 255
        assert np.array_equal(want[y0, x0:x0 + 13], canvas[y0, x0:x0 + 13]) and np.array_equal(want[y0 + 1, x0:x0 + 13], tile[1])
    from lightdiffusion_amd._lib import LDError
    with pytest.raises(LDError):                                                 # a region that leaves the canvas is refused, not clipped
        ops.u8_composite_(dev(canvas), dev(tile), dev(alpha), canvas.shape[1] - 5, 0)


def test_conversions():
    k = np.arange(256, dtype=np.float32) / np.float32(255.0)
    up, down = np.nextafter(k, np.float32(2)), np.nextafter(k, np.float32(-1))
    x = np.concatenate([k, up, down, np.array([-3.0, -1e-9, 1.0000001, 7.5, 0.5], np.float32)])     # k / 255 +- 1 ulp, negatives, above 1
    same(ops.u8_from_f32(dev(x)), R.to_u8(x), "fp32 -> u8")
    same(ops.u8_from_f32(dev(x)[1:]), R.to_u8(x[1:]), "fp32 -> u8, unaligned")
    b = np.arange(256, dtype=np.uint8)
    got = ops.f32_from_u8(dev(b)).cpu().numpy()
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), R.to_f32(b).view(np.uint32))      # a division, bit for bit
    assert np.array_equal(ops.f32_from_u8(dev(b)[3:250]).cpu().numpy(), R.to_f32(b[3:250]))


# ------------------------------------------------------------------ the ops beyond one lap of their grid-stride loops, and their other paths
# Every kernel of image.hip is a grid-stride loop of at most 4096 blocks of 256 lanes: LAP work items are one lap, and a 2048^2 canvas laps them
# several times.  Each case below passes LAP items by a few rows, so a wrong stride shows in the rows of the second lap; the other axis is short.
LAP = 4096 * 256

KERNELS = {
    "resample_h_kernel": ["test_resample", "test_resample_h_second_lap", "test_resample_channels_and_long_taps"],
    "resample_v_kernel": ["test_resample", "test_resample_v_second_lap", "test_resample_channels_and_long_taps", "test_resample_v_alignment_paths"],
    "box_h_kernel": ["test_blur", "test_blur_and_mask_second_lap", "test_blur_radius_beyond_the_image_and_in_place"],
    "box_v_kernel": ["test_blur", "test_blur_and_mask_second_lap", "test_blur_radius_beyond_the_image_and_in_place"],
    "mask_kernel": ["test_blur_weights_and_window", "test_blur_and_mask_second_lap", "test_mask_pattern_over_the_left_and_top_edges"],
    "composite_kernel": ["test_composite", "test_composite_second_lap"],
    "u8_from_f32_kernel": ["test_conversions", "test_conversions_second_lap"],
    "f32_from_u8_kernel": ["test_conversions", "test_conversions_second_lap"],
}


def same_at(got, want, what):
    """Byte for byte, naming the first differing pixel."""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{what}: {len(bad)} differing bytes, the first at {tuple(int(v) for v in bad[0])}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}"


def rand_u8(seed, shape):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def test_composite_second_lap():
    h, w = 1025, 1024                                                            # 1 049 600 pixels: LAP and one row
    assert h * w > LAP
    canvas, tile, alpha = rand_u8(20, (h + 2, w + 3, 3)), rand_u8(21, (h, w, 3)), rand_u8(22, (h, w))
    got = ops.u8_composite_(dev(canvas), dev(tile), dev(alpha), 3, 2)
    same_at(got, R.composite(canvas.copy(), tile, alpha, 3, 2), "composite 1025 x 1024 x 3")


def test_blur_and_mask_second_lap():
    h = w = 2052                                                                 # 513 words a row: 1 052 676 items, LAP and eight rows
    assert h * ((w + 3) // 4) > LAP
    pat = rand_u8(23, (2040, 2040))
    mask = ops.u8_mask(h, w, (7, 9, 2040, 2040), dev(pat))
    want = np.zeros((h, w), np.uint8)
    want[9:2049, 7:2047] = pat
    same_at(mask, want, "mask 2052 x 2052")
    same_at(ops.u8_gaussian_blur(mask, 2.5), R.gaussian_blur(want, 2.5), "blur 2052 x 2052, radius 2.5")


def test_resample_h_second_lap():
    src = rand_u8(24, (1024, 64, 3))                                             # 1024 rows of 64 -> 1025 pixels: 1 049 600 items
    assert 1024 * 1025 > LAP
    same_at(ops.u8_resample(dev(src), (1025, 1024)), R.resample(src, 1025, 1024), "horizontal resample 1024 x (64 -> 1025) x 3")


def test_resample_v_second_lap():
    src = rand_u8(25, (64, 1024, 3))                                             # 64 -> 1367 rows of 768 words: 1 049 856 items
    assert 1367 * (1024 * 3 // 4) > LAP
    same_at(ops.u8_resample(dev(src), (1024, 1367)), R.resample(src, 1024, 1367), "vertical resample (64 -> 1367) x 1024 x 3")


def test_conversions_second_lap():
    n = 4 * LAP + 3                                                              # four elements a lane: one full lap and a ragged word of the second
    rng = np.random.default_rng(26)
    x = (rng.random(n, dtype=np.float32) * np.float32(1.2) - np.float32(0.1))
    same_at(ops.u8_from_f32(dev(x)), R.to_u8(x), "fp32 -> u8, 4 LAP + 3 elements")
    b = rand_u8(27, (n,))
    got = ops.f32_from_u8(dev(b)).cpu().numpy()
    same_at(got.view(np.uint32), R.to_f32(b).view(np.uint32), "u8 -> fp32, 4 LAP + 3 elements")


@pytest.mark.parametrize("c,shape,size,filt", [(2, (37, 53), (72, 24), "lanczos"), (4, (37, 53), (72, 24), "lanczos"), (2, (33, 29), (11, 50), "bicubic"),
                                               (4, (40, 31), (17, 55), "bicubic"), (3, (64, 96), (12, 8), "lanczos"), (4, (64, 96), (12, 8), "lanczos")])
def test_resample_channels_and_long_taps(c, shape, size, filt):
    """Two and four channels, and an 8x lanczos downscale (49 taps a sample: the longest rows)."""
    src = rand_u8(30 + c + size[0], shape + (c,))
    same_at(ops.u8_resample(dev(src), size, filt), R.resample(src, size[0], size[1], filt), f"resample {shape} x {c} -> {size} {filt}")


def _resample_v_into(src_view, dst_view, filt="lanczos"):
    """The vertical pass alone (the width does not change) from one uint8 view into another, through the C ABI."""
    from lightdiffusion_amd._lib import check, lib
    sp, spitch, h, w, c = ops._u8_image(src_view)
    dp, dpitch, oh, ow, dc = ops._u8_image(dst_view)
    assert (w, c) == (ow, dc) and oh != h
    vco, vk = ops._coeffs_on(src_view.device, h, oh, filt)
    check(lib().ld_op_u8_resample(sp, spitch, w, h, c, dp, dpitch, ow, oh, None, 0, vco.data_ptr(), vk, None, torch.cuda.current_stream().cuda_stream), "ld_op_u8_resample")


@pytest.mark.parametrize("src_off,dst_off", [(0, 1), (1, 0), (3, 3), (0, 0)], ids=lambda v: str(v))
def test_resample_v_alignment_paths(src_off, dst_off):
    """resample_v_kernel moves a word per lane where pointer and pitch allow and bytes where they do not, separately for source and destination:
    an aligned source into a window at an odd byte offset of a larger tensor, the reverse, both unaligned, both aligned.  The bytes around the
    destination window stay as they were."""
    h, oh, w = 23, 37, 50                                                        # 50 bytes a row: twelve words and a ragged one
    big = rand_u8(40 + src_off, (h, 64))
    src = big[:, src_off:src_off + w]
    canvas = rand_u8(41 + dst_off, (oh + 2, 64))
    d = dev(canvas)
    _resample_v_into(dev(big)[:, src_off:src_off + w], d[1:1 + oh, dst_off:dst_off + w])
    want = canvas.copy()
    want[1:1 + oh, dst_off:dst_off + w] = R.resample(src, w, oh)
    same_at(d, want, f"vertical resample, source offset {src_off}, destination offset {dst_off}")


def _blur_into(src_view, dst_view, radius):
    from lightdiffusion_amd._lib import check, lib
    sp, spitch, h, w, _ = ops._u8_image(src_view)
    dp, dpitch, dh, dw, _ = ops._u8_image(dst_view)
    assert (h, w) == (dh, dw)
    tmp = torch.empty(lib().ld_op_u8_blur_tmp_bytes(w, h), dtype=torch.uint8, device=src_view.device)
    check(lib().ld_op_u8_gaussian_blur(sp, spitch, dp, dpitch, w, h, float(radius), tmp.data_ptr(), torch.cuda.current_stream().cuda_stream), "ld_op_u8_gaussian_blur")


@pytest.mark.parametrize("h,w", [(9, 50), (50, 9), (7, 5)])
def test_blur_radius_beyond_the_image_and_in_place(h, w):
    """Radius 16 is a box radius of 15: beyond the width - 1, the height - 1 or both, so every tap of some pass is the clamped border.  Then the
    same blur in place (dst is src), in a window at an odd offset of a larger tensor whose other bytes must not change."""
    assert ops.u8_box_weights(16)[0] == 15 and 15 >= min(h, w) - 1
    mask = rand_u8(50 + h, (h, w))
    want = R.gaussian_blur(mask, 16)
    same_at(ops.u8_gaussian_blur(dev(mask), 16), want, f"blur {h} x {w}, radius 16")
    canvas = rand_u8(51 + h, (h + 4, w + 9))
    canvas[2:2 + h, 5:5 + w] = mask
    d = dev(canvas)
    win = d[2:2 + h, 5:5 + w]
    _blur_into(win, win, 16)
    canvas[2:2 + h, 5:5 + w] = want
    same_at(d, canvas, f"blur {h} x {w} in place, radius 16")


def test_mask_pattern_over_the_left_and_top_edges():
    pat = rand_u8(60, (30, 41))
    for (h, w, x, y) in [(25, 33, -7, -4), (25, 33, -7, 3), (25, 33, 5, -29), (10, 10, -3, -2)]:
        want = np.zeros((h, w), np.uint8)
        y1, y2, x1, x2 = max(y, 0), min(y + 30, h), max(x, 0), min(x + 41, w)
        want[y1:y2, x1:x2] = pat[y1 - y:y2 - y, x1 - x:x2 - x]
        same_at(ops.u8_mask(h, w, (x, y, 41, 30), dev(pat)), want, f"mask {h} x {w}, pattern at ({x}, {y})")
        want[y1:y2, x1:x2] = 255
        same_at(ops.u8_mask(h, w, (x, y, 41, 30), None, DEV), want, f"mask {h} x {w}, rectangle at ({x}, {y})")


# ------------------------------------------------------------------ the node
@pytest.mark.parametrize("tag", ["b1", "b2"])
def test_node_with_standin_stages_reproduces_reference(flow_golden, tag):
    run_flow(flow_golden, tag, ops, DEV)


def usdu_kwargs(**over):
    kw = dict(S.flow_params(), seed=5, steps=2, cfg=3.0, sampler_name="euler_ancestral", scheduler="normal", force_uniform_tiles="enable")
    kw.update(over)
    return kw


def reference_loop(image, model, pos, neg, vae, upscaler, kw):
    """The same run written from usdu_ref (host, NumPy) and the package's existing nodes, in the reference's order (LD.py:8236-8324,
    7629-7739).  -> (uint8 canvas after the upscale, final uint8 canvas, crops)"""
    tw, th = kw["tile_width"], kw["tile_height"]
    batch = [R.to_u8(im.numpy()) for im in image]
    size = W, H = usdu.canvas_size(image.shape[2], image.shape[1], kw["upscale_by"])
    for _ in usdu.get_factors(-(-max(W, H) // max(image.shape[1:3]))):
        batch = [R.to_u8(N.ImageUpscaleWithModel().upscale(upscaler, torch.from_numpy(R.to_f32(im))[None])[0][0].numpy()) for im in batch]
    canvas = np.stack([R.resample(im, W, H) for im in batch])
    start = canvas.copy()
    grad = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 256, axis=1)
    row, col = np.zeros((th, tw), np.uint8), np.zeros((th, tw), np.uint8)
    row[:th // 2], row[th // 2:] = R.resample(grad, tw, th // 2, "bicubic"), R.resample(grad[::-1], tw, th // 2, "bicubic")
    col[:, :tw // 2], col[:, tw // 2:] = R.resample(grad.T, tw // 2, th, "bicubic"), R.resample(grad.T[:, ::-1], tw // 2, th, "bicubic")
    crops = []
    for kind, px, py in usdu.jobs(size, tw, th, True, True):
        mask = np.zeros((H, W), np.uint8)
        if kind == "redraw":
            tile, pad, blur = usdu.redraw_tile_size(tw, th, kw["tile_padding"]), kw["tile_padding"], kw["mask_blur"]
            mask[py:py + th + 1, px:px + tw + 1] = 255
        else:
            tile, pad, blur = (tw, th), kw["seam_fix_padding"], kw["seam_fix_mask_blur"]
            pat = row if kind == "row" else col
            mask[py:py + th, px:px + tw] = pat[:H - py, :W - px]
        ys, xs = np.nonzero(mask)
        x1, y1, x2, y2 = crop = usdu.job_crop((xs.min(), ys.min(), xs.max() + 1, ys.max() + 1), pad, size, tile)
        crops.append(crop)
        alpha = R.gaussian_blur(mask, blur)[y1:y2, x1:x2]
        tiles = np.stack([R.resample(c[y1:y2, x1:x2], tile[0], tile[1]) for c in canvas])
        lat = N.VAEEncode().encode(vae, torch.from_numpy(R.to_f32(tiles)))[0]
        lat = N.KSampler2().sample(model, kw["seed"], kw["steps"], kw["cfg"], kw["sampler_name"], kw["scheduler"], pos, neg, lat, denoise=kw["denoise"])[0]
        dec = R.to_u8(N.VAEDecode().decode(vae, lat)[0].numpy())
        for b in range(len(canvas)):
            R.composite(canvas[b], R.resample(dec[b], x2 - x1, y2 - y1), alpha, x1, y1)
    return start, canvas, crops


def test_node_with_real_stages_equals_the_loop_on_existing_nodes():
    """Expected: identical bytes.  The stages are the package's existing nodes on both sides, the seeds are the same and the posterior and
    sampler noise come from the host generator in the same order, so the only difference is where the 8-bit plumbing runs.  The loop below
    is run twice first: should the existing stages not be run-to-run deterministic, that figure (and only that) is the allowance.
    Measured on the MI355X: the loop's two runs differ in 0 bytes, and the node differs from it in 0 bytes."""
    model, clip, vae = N.load_synthetic(DEV, max_batch=1, max_hw=(8, 8), tiny=True)
    upscaler = N.load_synthetic_upscaler(DEV, nb=1)
    enc = lambda t: clip.encode_from_tokens(t, return_pooled=True)
    (pc, pp) = enc(TOKS)
    pos = neg = [[pc, {"pooled_output": pp}]]
    image, kw = S.flow_input(1), usdu_kwargs()
    torch.manual_seed(11)
    start, ref1, crops = reference_loop(image, model, pos, neg, vae, upscaler, kw)
    torch.manual_seed(11)
    _, ref2, _ = reference_loop(image, model, pos, neg, vae, upscaler, kw)
    noise = int(np.abs(ref1.astype(int) - ref2.astype(int)).max())
    print(f"run-to-run difference of the test-side loop: {noise} (uint8 steps)")
    torch.manual_seed(11)
    (out,) = N.UltimateSDUpscale().upscale(image, model, pos, neg, vae, upscale_model=upscaler, **kw)
    assert tuple(out.shape) == (1, 96, 80, 3) and out.device.type == "cpu" and out.dtype == torch.float32
    got = S.as_u8(out)
    diff = int(np.abs(got.astype(int) - ref1.astype(int)).max())
    print(f"node vs test-side loop: max difference {diff}, {int((got != ref1).sum())} differing bytes")
    assert diff <= noise
    assert np.array_equal(out.numpy(), R.to_f32(got))
    for (x1, y1, x2, y2) in crops[:9]:                                           # the redraw ran: every tile differs from the plain upscale
        assert (got[:, y1:y2, x1:x2] != start[:, y1:y2, x1:x2]).any()


def test_img2img_one_full_size_job():
    """272 x 272 -> a 544 x 544 canvas with the reference's constants (tile 512, padding 32): redraw tiles of 544^2 (68 x 68 latents:
    68 -> 34 -> 17 -> 9 in the UNet), each crop the whole canvas.  ceil(544 / 512) = 2, so the grid is 2 x 2: four such redraw jobs and four
    512^2 seam jobs, not one job."""
    model, clip, vae = N.load_synthetic(DEV, max_batch=1, max_hw=(68, 68))
    upscaler = N.load_synthetic_upscaler(DEV, nb=1)
    image = torch.rand(1, 272, 272, 3, generator=torch.Generator().manual_seed(0))
    out = N.img2img(model, clip, vae, upscaler, image, TOKS, TOKS, seed=3, steps=2, sampler_name="euler_ancestral", scheduler="normal")
    assert tuple(out.shape) == (1, 544, 544, 3) and out.dtype == torch.float32
    assert torch.isfinite(out).all() and float(out.min()) >= 0.0 and float(out.max()) <= 1.0
    torch.cuda.synchronize()                                                     # no launch left an error behind
