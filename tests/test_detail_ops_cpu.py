"""CPU: what the device tests of the Detailer's fp32 image kernels (tests/test_detail_ops_gpu.py) rest on.
  * `blur_restated`: gauss_axis_kernel's arithmetic written out in torch fp32 — the host's taps (ops.gaussian_taps), a pass along x, then a pass
    along y, acc = acc + tap[j] * in[reflect(i + j - feather)] with j ascending from 0 and the product and the sum each rounded to fp32.  Held
    here to the fp64 blur within detailer_ref.blur_bound on every case; the device test holds the kernel to it bit for bit.
  * the bitwise paste test has teeth: a sum contracted into one FMA, and a reciprocal multiply for / 255, both give other bits."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detailer_ref as R            # noqa: E402
import detailer_standins as S       # noqa: E402
from lightdiffusion_amd import ops  # noqa: E402

LAP_BLUR = (1030, 1030, 5)          # (H, W, feather): more than the 4096 x 256 lanes of one lap of the kernel's grid-stride loop


def lap_mask():
    h, w, _ = LAP_BLUR
    return np.random.default_rng(5).random((h, w), dtype=np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def blur_restated(mask, feather, sigma=10.0):
    """[H, W] fp32 array -> [H, W] fp32 array, in gauss_axis_kernel's order of operations (module docstring)."""
    a = torch.from_numpy(np.ascontiguousarray(mask, np.float32))
    if feather == 0:
        return a.numpy().copy()
    taps = ops.gaussian_taps(feather, sigma)
    assert taps.dtype == torch.float32 and tuple(taps.shape) == (2 * feather + 1,)

    def along_last(x):
        n = x.shape[1]
        idx = torch.arange(n)
        acc = torch.zeros_like(x)
        for j in range(2 * feather + 1):
            src = torch.from_numpy(R.reflect_index(idx.numpy() + j - feather, n))
            acc = acc + taps[j] * x[:, src]                # two fp32 roundings: the product, then the sum
        return acc
    return along_last(along_last(a).T.contiguous()).T.contiguous().numpy()


def test_host_taps_are_torchvisions():
    """linspace(-f, f, 2 f + 1), exp(-0.5 (x / sigma)^2), divided by their sum, all in fp32 — against the same in fp64."""
    for feather in (1, 5, 20, 100, 127):
        t = ops.gaussian_taps(feather, 10.0)
        assert t.dtype == torch.float32 and len(t) == 2 * feather + 1
        assert float(np.abs(t.double().numpy() - R.gaussian_taps(feather, 10.0)).max()) <= 2.0 ** -23 * float(t.max())
    assert float(ops.gaussian_taps(0, 10.0)) == 1.0


@pytest.mark.parametrize("h,w,feather", S.BLUR_CASES + [LAP_BLUR])
def test_restated_tap_order_stays_inside_the_blur_bound(h, w, feather):
    mask = S.blur_mask(h, w, feather) if (h, w, feather) != LAP_BLUR else lap_mask()
    got = blur_restated(mask, feather)
    err = float(np.abs(got.astype(np.float64) - R.gaussian_blur(mask, feather)).max())
    print(f"blur {S.blur_name(h, w, feather)}: fp32 in the kernel's order vs fp64 {err:.3e}, bound {R.blur_bound(feather):.3e}")
    assert got.dtype == np.float32 and err <= R.blur_bound(feather)
    if feather == 0:
        assert np.array_equal(bits(got), bits(mask))


def test_restatement_is_not_the_fp64_blur_rounded():
    """The order matters at the last bit: the device test's bitwise comparison with the restatement says more than its bound does."""
    h, w, feather = 65, 130, 5
    mask = S.blur_mask(h, w, feather)
    assert not np.array_equal(bits(blur_restated(mask, feather)), bits(R.gaussian_blur(mask, feather).astype(np.float32)))


# ------------------------------------------------------------------ the paste's roundings
def paste_contracted(canvas, tile, alpha, x0, y0):
    """detailer_ref.paste with the sum contracted: fma(1 - a, canvas, a * t), the product (1 - a) * canvas exact (fp64 holds it) and one rounding
    of the sum to fp32."""
    H, W = canvas.shape[:2]
    h, w = min(H, y0 + tile.shape[0]) - y0, min(W, x0 + tile.shape[1]) - x0
    a = np.asarray(alpha, np.float32)[:h, :w, None]
    win = canvas[y0:y0 + h, x0:x0 + w]
    second = a * R.to_f32(tile[:h, :w])                                                   # fp32, rounded
    canvas[y0:y0 + h, x0:x0 + w] = ((np.float32(1.0) - a).astype(np.float64) * win.astype(np.float64) + second.astype(np.float64)).astype(np.float32)
    return canvas


@pytest.mark.parametrize("name", list(S.PASTE_CASES))
def test_a_contracted_paste_gives_other_bits(name):
    x0, y0, _ = S.PASTE_CASES[name]
    tile, alpha = S.paste_inputs(name)
    want = R.paste(S.paste_canvas(), tile, alpha, x0, y0)
    got = paste_contracted(S.paste_canvas(), tile, alpha, x0, y0)
    n = int((bits(got) != bits(want)).sum())
    print(f"paste {name}: {n} of {want.size} floats differ under contraction")
    assert n >= 1
    assert float(np.abs(got.astype(np.float64) - want).max()) <= 2.0 ** -22          # ... by an ulp or so: only a bitwise test sees it


def test_a_reciprocal_multiply_is_not_the_division():
    k = np.arange(256, dtype=np.float32)
    div = k / np.float32(255.0)
    mul = k * (np.float32(1.0) / np.float32(255.0))
    assert div.dtype == mul.dtype == np.float32 and np.array_equal(bits(div), bits(R.to_f32(np.arange(256, dtype=np.uint8))))
    n = int((bits(div) != bits(mul)).sum())
    print(f"{n} of 256 byte values differ between k / 255 and k * (1 / 255)")
    assert n >= 1
