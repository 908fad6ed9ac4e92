"""fp64 model of the nearest-2x fold (helper module of the upconv tests): the 3x3 convolution of a 2x-upsampled image as four 2x2
convolutions of the source image, one per output phase (py, px).

Output pixel (2y + py, 2x + px) reads the source pixels (y + py - 1 + a, x + px - 1 + b), a, b in {0, 1}.  Per axis the 3x3 taps that fall
on source offset a are TAPS[(phase, a)]: phase 0 — a = 0 takes tap 0, a = 1 taps 1 and 2; phase 1 — a = 0 takes taps 0 and 1, a = 1 tap 2.
Zero padding carries over: source row -1 / row H stand for upsampled rows -1 / 2H.
"""
import torch

TAPS = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}


def fold_weights(w_oihw: torch.Tensor) -> torch.Tensor:
    """[O][I][3][3] -> [py][px][a][b][O][I]: every phase-tap matrix as the sum of its 3x3 taps (in the dtype of w)."""
    O, I = w_oihw.shape[:2]
    out = torch.zeros(2, 2, 2, 2, O, I, dtype=w_oihw.dtype, device=w_oihw.device)
    for py in (0, 1):
        for px in (0, 1):
            for a in (0, 1):
                for b in (0, 1):
                    for ky in TAPS[(py, a)]:
                        for kx in TAPS[(px, b)]:
                            out[py, px, a, b] += w_oihw[:, :, ky, kx]
    return out


def is_sum(py: int, px: int, a: int, b: int) -> bool:
    """Is phase-tap (py, px, a, b) a sum of several 3x3 taps (12 of the 16 are)?"""
    return len(TAPS[(py, a)]) * len(TAPS[(px, b)]) > 1


def phase_operands(x_nhwc: torch.Tensor, wf: torch.Tensor, py: int, px: int, only_sums: bool = False):
    """The contraction of one phase: A [n h w][4 C] (taps (a, b) of the zero-padded source, tap-major) and W [O][4 C].
    only_sums: the columns of single-tap phase-taps are zeroed (the operands of the fold's rounding term)."""
    n, h, w, c = x_nhwc.shape
    xp = torch.nn.functional.pad(x_nhwc, (0, 0, 1, 1, 1, 1))
    cols, ws = [], []
    for a in (0, 1):
        for b in (0, 1):
            keep = 1.0 if (not only_sums or is_sum(py, px, a, b)) else 0.0
            cols.append(xp[:, py + a:py + a + h, px + b:px + b + w, :].reshape(n * h * w, c) * keep)
            ws.append(wf[py, px, a, b])
    return torch.cat(cols, 1), torch.cat(ws, 1)


def interleave(phases, n: int, h: int, w: int) -> torch.Tensor:
    """{(py, px): [n h w][O]} -> [n][2h][2w][O] (depth to space)."""
    O = phases[(0, 0)].shape[-1]
    out = torch.empty(n, 2 * h, 2 * w, O, dtype=phases[(0, 0)].dtype, device=phases[(0, 0)].device)
    for (py, px), t in phases.items():
        out[:, py::2, px::2, :] = t.reshape(n, h, w, O)
    return out
