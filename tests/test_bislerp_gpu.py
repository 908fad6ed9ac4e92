"""GPU: bislerp_axis_kernel (misc.hip) through ops.bislerp, each of its two passes held element-wise (tests/errbound.py bislerp_axis_ref) against
the fp64 slerp of the same fp32 inputs: the width pass against the input, the height pass against the DEVICE's own width-pass output taken as
exact.  Random latents reach only the general arm of the reference (LD.py:429-463), so every case plants one tap pair per special arm — a zero tap on
either side and on both, b = 2a (copied), b = -a (lerped), a right angle, and dot = +-(1 - 1e-3) next to the poles — and asserts those outputs by
value as well.  Each case prints its worst error / bound and signed bias per pass.

KERNELS names the tests that hold the kernel (tests/test_errbound_cpu.py keeps the ledger); cases() and make_input() are also what the CPU
self-check of the reference runs the oracle's fp32 bislerp through."""
import math

import pytest
import torch

import errbound as EB

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

KERNELS = {"bislerp_axis_kernel": ["test_bislerp_passes", "test_bislerp_rejects"]}

# (h, w, h_new, w_new): 2x; ragged; a downscale; an axis that does not change on a one-pixel-high image; a one-pixel-wide image.  All at batch 2.
SHAPES = [(6, 5, 12, 10), (6, 5, 9, 11), (8, 8, 5, 3), (1, 7, 1, 7), (7, 1, 14, 1)]
KINDS = ["a0", "b0", "both0", "double", "neg", "near-1", "near+1", "perp"]
NEAR = 1.0 - 1e-3


def cases():
    return [(c, h, w, hn, wn) for c in (4, 1) for (h, w, hn, wn) in SHAPES]


def _pairs(len_old, len_new):
    """Tap pairs (lo, lo + 1) the resize uses, none sharing a pixel with another."""
    from oracle import sd15_ref as O
    lo, hi, _ = O._bilinear_taps(len_old, len_new)
    out, last = [], -2
    for l, h in sorted(set(zip(lo.tolist(), hi.tolist()))):
        if h == l + 1 and l >= last + 2:
            out.append(l)
            last = l
    return out


def _plant(kind, a, g):
    """(a, b) of one planted pair from the random C-vector a (C = 1: the kinds that need a second direction do not exist)."""
    c = a.numel()
    if kind == "a0":
        return torch.zeros_like(a), a
    if kind == "b0":
        return a, torch.zeros_like(a)
    if kind == "both0":
        return torch.zeros_like(a), torch.zeros_like(a)
    if kind == "double":
        return a, 2.0 * a
    if kind == "neg":
        return a, -a
    if c == 1:
        return None
    p = torch.randn(c, generator=g, dtype=torch.float64)
    ad = a.double()
    p = p - (p @ ad) / (ad @ ad) * ad                      # orthogonal to a
    p = p / p.norm() * ad.norm()
    cos = {"perp": 0.0, "near+1": NEAR, "near-1": -NEAR}[kind]
    return a, (1.5 * (cos * ad + math.sqrt(1.0 - cos * cos) * p)).float()


def make_input(c, h, w, hn, wn, n=2):
    """-> (x fp32 [n][c][h][w], plants = [(kind, image, row, column or None, lo)]): pairs along the width where the width has tap pairs, else along
    the height (a one-pixel-wide image passes the width pass unchanged, so the height pass meets them)."""
    g = torch.Generator().manual_seed(1000 * c + 100 * h + 10 * w + hn + wn)
    x = torch.randn(n, c, h, w, generator=g)
    along_w = w > 1
    pairs = _pairs(w, wn) if along_w else _pairs(h, hn)
    lines = [(i, r) for i in range(n) for r in range(h if along_w else w)]
    slots = [(i, r, lo) for lo in pairs for (i, r) in lines]
    plants = []
    for kind, (i, r, lo) in zip(KINDS, slots):
        ab = _plant(kind, x[i, :, r, lo] if along_w else x[i, :, lo, r], g)
        if ab is None:
            continue
        if along_w:
            x[i, :, r, lo], x[i, :, r, lo + 1] = ab
        else:
            x[i, :, lo, r], x[i, :, lo + 1, r] = ab
        plants.append((kind, i, r, along_w, lo))
    return x, plants


def planted_value(kind, a, b, r):
    """What the reference's arms make of a planted pair, in closed form (fp64)."""
    a, b = a.double(), b.double()
    if kind == "a0":
        return r * math.sin(r * math.pi / 2) * b            # ua = 0, dot = 0: om = pi / 2, magnitude nb r
    if kind == "b0":
        return (1 - r) * math.sin((1 - r) * math.pi / 2) * a
    if kind == "both0":
        return torch.zeros_like(a)
    if kind == "double":
        return a
    if kind == "neg":
        return a * (1 - r) + b * r
    return None


def check_planted(y, x, plants, len_new, axis_w, what):
    """The outputs of the planted pairs along this pass's axis, by value: the copy and the zero bit for bit, the closed forms to 1e-6 of |a| + |b|."""
    from oracle import sd15_ref as O
    len_old = x.shape[3] if axis_w else x.shape[2]
    lo, hi, fr = O._bilinear_taps(len_old, len_new)
    seen = set()
    for kind, i, line, along_w, l in plants:
        if along_w != axis_w:
            continue
        for o in [o for o in range(len_new) if int(lo[o]) == l and int(hi[o]) == l + 1]:
            r = float(fr[o])
            if axis_w:
                a, b, got = x[i, :, line, l], x[i, :, line, l + 1], y[i, :, line, o]
            else:
                a, b, got = x[i, :, l, line], x[i, :, l + 1, line], y[i, :, o, line]
            want = planted_value(kind, a.cpu(), b.cpu(), r)
            seen.add(kind)
            if want is None:
                continue
            got = got.cpu().double()
            if kind in ("double", "both0"):
                assert torch.equal(got, want), f"{what}: planted {kind} at image {i}, line {line}, output {o}: got {got.tolist()}, want {want.tolist()}"
            else:
                assert bool(((got - want).abs() <= 1e-6 * (a.cpu().double().abs() + b.cpu().double().abs())).all()), \
                    f"{what}: planted {kind} at image {i}, line {line}, output {o} (r = {r:.4f}): got {got.tolist()}, want {want.tolist()}"
    return seen


@pytest.fixture(scope="module")
def ops():
    from lightdiffusion_amd import ops as o
    from lightdiffusion_amd._lib import lib
    lib()
    return o


def held(y, ref, bound, what):
    r, s = EB.check(y, ref, bound, what, keep=torch.ones_like(ref, dtype=torch.bool), bias_extra=EB.rtn_noise(ref.numel()))
    print(f"{what}: error / bound {r:.3f}, signed bias {s:+.2e}")
    return r, s


@pytest.mark.parametrize("c,h,w,hn,wn", cases(), ids=lambda v: str(v))
def test_bislerp_passes(ops, c, h, w, hn, wn):
    x, plants = make_input(c, h, w, hn, wn)
    xd = x.to(DEV)
    tmp = torch.full((2, c, h, wn), float("nan"), dtype=torch.float32, device=DEV)
    y = ops.bislerp(xd, wn, hn, tmp=tmp)
    assert tuple(y.shape) == (2, c, hn, wn) and y.dtype == torch.float32
    what = f"bislerp C={c} {h}x{w} -> {hn}x{wn}"
    ref1, b1, dot1 = EB.bislerp_axis_ref(x, wn, True)
    assert EB.bislerp_dots_clear_of_the_thresholds(dot1), f"{what}: a width pair stands at the branch threshold; change the inputs"
    held(tmp.cpu(), ref1, b1, what + " width pass")
    t = tmp.cpu()
    ref2, b2, dot2 = EB.bislerp_axis_ref(t, hn, False)
    assert EB.bislerp_dots_clear_of_the_thresholds(dot2), f"{what}: a height pair stands at the branch threshold; change the inputs"
    held(y.cpu(), ref2, b2, what + " height pass")
    seen = check_planted(t, x, plants, wn, True, what + " width pass") | check_planted(y.cpu(), t, plants, hn, False, what + " height pass")
    assert seen == {k for k, *_ in plants} and len(seen) >= 3, (what, sorted(seen))
    if c == 4 and h * w >= 30:
        assert seen == set(KINDS), (what, sorted(seen))
    print(f"{what}: planted arms {sorted(seen)}")


def test_bislerp_rejects(ops):
    from lightdiffusion_amd._lib import ERR_ARG, LDError
    x = torch.zeros(1, 4, 3, 3, device=DEV)
    for width, height in ((0, 3), (3, 0)):
        with pytest.raises(LDError) as e:
            ops.bislerp(x, width, height)
        assert e.value.status == ERR_ARG
