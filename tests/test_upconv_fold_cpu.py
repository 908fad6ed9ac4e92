"""The algebra of the nearest-2x fold, without a GPU: four 2x2 convolutions of the source image with the 16 phase-tap matrices of
tests/upconv_ref.py equal the 3x3 convolution of the nearest-upsampled image (fp64, 1e-12)."""
import torch
import torch.nn.functional as F

import upconv_ref as UR


def test_phase_table_matches_upsample_then_conv():
    g = torch.Generator().manual_seed(0)
    n, c, o, h, w = 2, 5, 7, 6, 9                                   # non-square, odd width
    x = torch.randn(n, c, h, w, generator=g, dtype=torch.float64)
    wt = torch.randn(o, c, 3, 3, generator=g, dtype=torch.float64)
    want = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), wt, padding=1)
    wf = UR.fold_weights(wt)
    got = torch.empty_like(want)
    for py in (0, 1):
        for px in (0, 1):
            # a 2x2 convolution over the source padded by one pixel: window (y + py + a, x + px + b) of the padded image
            k = wf[py, px].permute(2, 3, 0, 1)                        # [O][I][a][b]
            full = F.conv2d(F.pad(x, (1, 1, 1, 1)), k)                # [n][O][h + 1][w + 1]: windows starting at every padded pixel
            got[:, :, py::2, px::2] = full[:, :, py:py + h, px:px + w]
    assert float((got - want).abs().max()) <= 1e-12


def test_phase_operands_are_the_same_contraction():
    """The [rows][4 C] x [O][4 C] form the kernel runs (upconv_ref.phase_operands) gives the same numbers, NHWC, depth-to-space interleaved."""
    g = torch.Generator().manual_seed(1)
    n, c, o, h, w = 3, 4, 6, 5, 3
    x = torch.randn(n, h, w, c, generator=g, dtype=torch.float64)
    wt = torch.randn(o, c, 3, 3, generator=g, dtype=torch.float64)
    want = F.conv2d(F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode="nearest"), wt, padding=1).permute(0, 2, 3, 1)
    wf = UR.fold_weights(wt)
    ph = {}
    for py in (0, 1):
        for px in (0, 1):
            A, Wm = UR.phase_operands(x, wf, py, px)
            ph[(py, px)] = A @ Wm.t()
    assert float((UR.interleave(ph, n, h, w) - want).abs().max()) <= 1e-12


def test_twelve_of_sixteen_phase_taps_are_sums():
    assert sum(UR.is_sum(py, px, a, b) for py in (0, 1) for px in (0, 1) for a in (0, 1) for b in (0, 1)) == 12
    ones = UR.fold_weights(torch.ones(1, 1, 3, 3, dtype=torch.float64))
    assert float(ones.sum()) == 36.0                                   # every 3x3 tap is used once per phase
    assert sorted(ones.flatten().tolist()) == [1.0] * 4 + [2.0] * 8 + [4.0] * 4
