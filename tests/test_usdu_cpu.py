"""UltimateSDUpscale without a GPU: the NumPy restatement of the image ops against Pillow and its recorded outputs, the geometry and the
whole job loop of lightdiffusion_amd.usdu against the reference's recorded run (tests/golden/usdu_flow.npz, tools/make_usdu_golden.py),
the rejections, and the package's independence from PIL."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import usdu_ref as R            # noqa: E402
import usdu_standins as S       # noqa: E402

GOLDEN = os.path.join(HERE, "golden")


@pytest.fixture(scope="module")
def ops_golden():
    return np.load(os.path.join(GOLDEN, "usdu_ops.npz"))


@pytest.fixture(scope="module")
def flow_golden():
    return np.load(os.path.join(GOLDEN, "usdu_flow.npz"))


def ref_resample(case):
    src, box, size, filt = case
    if box is not None:
        src = src[box[1]:box[3], box[0]:box[2]]
    return R.resample(src, size[0], size[1], filt)


def test_ref_equals_recorded_pillow(ops_golden):
    for name, case in S.resample_cases().items():
        assert np.array_equal(ref_resample(case), ops_golden["resample_" + name]), name
    for name, (mask, radius) in S.blur_cases().items():
        assert np.array_equal(R.gaussian_blur(mask, radius), ops_golden["blur_" + name]), name
    for name, (canvas, tile, alpha, x0, y0) in S.composite_cases().items():
        assert np.array_equal(R.composite(canvas.copy(), tile, alpha, x0, y0), ops_golden["composite_" + name]), name


def test_ref_equals_pillow_live():
    Image = pytest.importorskip("PIL.Image")
    ImageFilter = pytest.importorskip("PIL.ImageFilter")
    for name, (src, box, size, filt) in S.resample_cases().items():
        im = Image.fromarray(src)
        im = im if box is None else im.crop(box)
        want = np.array(im.resize(size, {"lanczos": Image.LANCZOS, "bicubic": Image.BICUBIC}[filt]))
        assert np.array_equal(ref_resample((src, box, size, filt)), want), name
    rng = np.random.default_rng(0)
    filt = {"lanczos": Image.LANCZOS, "bicubic": Image.BICUBIC}
    # four channels as CMYK and two as a pair of "L" bands (Pillow premultiplies LA and RGBA before it resizes them; its resampling itself
    # treats every band alike), up and down, and an 8x lanczos downscale: the longest tap rows
    for (h, w, c, size, f) in [(37, 53, 4, (72, 24), "lanczos"), (40, 31, 4, (17, 55), "bicubic"), (37, 53, 2, (72, 24), "lanczos"),
                               (33, 29, 2, (11, 50), "bicubic"), (64, 96, 3, (12, 8), "lanczos"), (64, 96, 4, (12, 8), "lanczos")]:
        src = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
        if c == 2:
            want = np.stack([np.array(Image.fromarray(src[..., k]).resize(size, filt[f])) for k in range(2)], axis=-1)
        else:
            want = np.array(Image.fromarray(src, "CMYK" if c == 4 else "RGB").resize(size, filt[f]))
        assert np.array_equal(R.resample(src, size[0], size[1], f), want), (h, w, c, size, f)
    # the last three: a radius beyond the image's width, its height, both
    for (h, w, r) in [(50, 70, 2.5), (96, 120, 16), (64, 64, 8), (20, 10, 16), (9, 50, 16), (50, 9, 16), (7, 5, 16)]:
        m = rng.integers(0, 256, (h, w), dtype=np.uint8)
        assert np.array_equal(R.gaussian_blur(m, r), np.array(Image.fromarray(m).filter(ImageFilter.GaussianBlur(r)))), (h, w, r)


def test_conversions():
    k = np.arange(256, dtype=np.uint8)
    f = R.to_f32(k)
    assert f.dtype == np.float32 and np.array_equal(R.to_u8(f), k)                     # k / 255 * 255 truncates back to k
    assert np.array_equal(R.to_u8(np.array([-0.5, 1.5, np.nextafter(np.float32(1.0), np.float32(0))], np.float32)), [0, 255, 254])


def test_geometry_reproduces_recorded_crops(flow_golden):
    from lightdiffusion_amd import usdu
    P = S.flow_params()
    tw, th, redraw, seams = usdu.check_arguments(P["mode_type"], P["seam_fix_mode"], P["tile_width"], P["tile_height"])
    size = usdu.canvas_size(40, 48, P["upscale_by"])
    assert size == (80, 96)
    row, col = usdu.seam_gradients(S.RefOps, tw, th, "cpu")
    jobs = usdu.jobs(size, tw, th, redraw, seams)
    assert len(jobs) == S.FLOW_JOBS == len(flow_golden["b1_crop"])
    for j, (kind, px, py) in enumerate(jobs):
        if kind == "redraw":
            tile, pad = usdu.redraw_tile_size(tw, th, P["tile_padding"]), P["tile_padding"]
            bbox = usdu.rectangle_bbox(px // tw, py // th, tw, th, size)
        else:
            tile, pad = (tw, th), P["seam_fix_padding"]
            bbox = usdu.pattern_bbox(row if kind == "row" else col, px, py, size)
        assert tuple(flow_golden["b1_tile_size"][j]) == tile, j
        assert tuple(flow_golden["b1_crop"][j]) == usdu.job_crop(bbox, pad, size, tile), (j, kind)


def run_flow(flow_golden, tag, ops, device):
    """The package's job loop with the stand-in stages; every job is compared with the reference's record as it happens."""
    from lightdiffusion_amd import usdu
    B = int(tag[1])
    expected = {"canvas": None, "jobs": 0}

    def observe(job):
        j = job.index
        x1, y1, x2, y2 = job.crop
        assert tuple(flow_golden[f"{tag}_crop"][j]) == tuple(job.crop) and tuple(flow_golden[f"{tag}_tile_size"][j]) == tuple(job.tile_size)
        assert np.array_equal(job.alpha.cpu().numpy(), flow_golden[f"{tag}_alpha_{j:02d}"]), f"blurred mask of job {j}"
        assert np.array_equal(job.tiles.cpu().numpy(), flow_golden[f"{tag}_tiles_{j:02d}"]), f"tiles handed to the encoder in job {j}"
        canvas = job.canvas.cpu().numpy()
        if expected["canvas"] is None:          # the canvas before the first job is known only inside its region afterwards
            expected["canvas"] = canvas.copy()
        expected["canvas"][:, y1:y2, x1:x2] = flow_golden[f"{tag}_after_{j:02d}"]       # outside the region nothing may change
        assert np.array_equal(canvas, expected["canvas"]), f"canvas after job {j}"
        expected["jobs"] += 1

    (out,) = usdu.upscale(S.flow_input(B), None, None, None, None, seed=1, steps=2, cfg=1.0, sampler_name="euler", scheduler="normal",
                          upscale_model=None, force_uniform_tiles="enable", stages=S.standin_stages(ops, device, observe), **S.flow_params())
    assert expected["jobs"] == S.FLOW_JOBS
    assert out.dtype == torch.float32 and out.device.type == "cpu"
    assert np.array_equal(S.as_u8(out), flow_golden[f"{tag}_final"])
    assert np.array_equal(out.numpy(), R.to_f32(flow_golden[f"{tag}_final"]))            # x / 255 exactly


@pytest.mark.parametrize("tag", ["b1", "b2"])
def test_job_loop_reproduces_reference(flow_golden, tag):
    run_flow(flow_golden, tag, S.RefOps, "cpu")


def test_rejections():
    from lightdiffusion_amd import usdu
    with pytest.raises(ValueError, match="LINEAR loop"):
        usdu.check_arguments("Chess", "None", 512, 512)
    for name in ("Band Pass", "Half Tile + Intersections"):
        with pytest.raises(ValueError, match="HALF TILE loop"):
            usdu.check_arguments("Linear", name, 512, 512)
    with pytest.raises(ValueError, match="expected one of"):
        usdu.check_arguments("Spiral", "None", 512, 512)
    with pytest.raises(ValueError, match="multiples of 8"):
        usdu.check_arguments("Linear", "Half Tile", 500, 512)
    assert usdu.check_arguments("Linear", "None", 500, 0) == (500, 500, True, False)     # a redraw tile is rounded up to 8 by itself
    assert usdu.check_arguments("None", "Half Tile", 64, 0) == (64, 64, False, True)
    assert usdu.get_factors(1) == [] and usdu.get_factors(2) == [2] and usdu.get_factors(4) == [4] and usdu.get_factors(6) == [3, 2]
    for bad in (5, 7, 10):
        with pytest.raises(ValueError, match="never terminates"):
            usdu.get_factors(bad)
    with pytest.raises(ValueError, match="never terminates"):                            # 64 -> 320: a scale factor of 5
        usdu.upscale(torch.zeros(1, 64, 64, 3), None, None, None, None, seed=0, steps=1, cfg=1.0, sampler_name="euler", scheduler="normal",
                     upscale_model=None, force_uniform_tiles="enable", stages=S.standin_stages(S.RefOps, "cpu"), **dict(S.flow_params(), upscale_by=5))


def test_package_imports_without_pil():
    code = ("import sys\nsys.modules['PIL'] = None\n"
            "import lightdiffusion_amd, lightdiffusion_amd.usdu, lightdiffusion_amd.nodes, lightdiffusion_amd.ops\n"
            "assert hasattr(lightdiffusion_amd.nodes, 'UltimateSDUpscale') and hasattr(lightdiffusion_amd.nodes, 'img2img')\n")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)
