"""The ResBlock 1x1 skip_connection as centre-only steps of the halo-tile convolution (conv6_kernel's skip segment, conv6.hip).

Every case drives the operator the UNet executor's second ResBlock half is (ld_op_conv_skip, and ld_op_groupnorm_conv_skip where out_layers'
GroupNorm is fused), first asserts by profile name that the launch ran on conv6_kernel (a case served by a tap-major kernel fails there: the
names differ), then holds EVERY output element to the bound of tests/errbound.py against the folded contraction in fp64 from the same fp16
inputs: columns [im2col(x) | s1 | s2] against weight rows [w | wskip], bias b + bskip — the construction and bound of
test_routes_gpu.py::test_conv_skip_route, plus 2^-11 |SiLU(GN(x))| |W|^T for the loader's one rounding of the normalised operand where the
GroupNorm is fused (test_groupnorm_conv_route).  The skip columns carry no such term: they enter raw.

Shapes: the smallest that gemm_plan's tile-count rule (v6_plan: 256 x 320 tiles x slices over K >= 192, slices only from 9 Cin >= 8640, at most
9 Cin / 2560 of them) still routes to conv6 —
  W64, N = 320:   16 tiles per image, unsplit below Cin = 960: n = 12 (192 tiles); Cin = 1024: n = 6 (96 tiles x 3 slices of 10 / 11 / 11 slabs)
  W16, N = 1280:  4 tiles per image x 4 slices: n = 12 (192 workgroups); Cin = 1344 gives slices of 10 / 11 / 10 / 11 slabs
  W32, N = 640:   8 tiles per image, unsplit (9 Cin = 5760): n = 24 (192 tiles) — the level-1 shape of a batch >= 12 pair / the hires step
Slab-count parity decides which halo buffer holds a workgroup's last slab (the skip images start in the other one); the skip step counts
20, 30, 10 (unsplit), 3 / 3 / 4 and 20 per slice cover both parities of the four-slot image ring as well.
"""
import math

import pytest
import torch

import errbound as EB

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    from lightdiffusion_amd import ops as o
    from lightdiffusion_amd._lib import lib
    lib()
    return o


def r16(shape, seed, scale=1.0, offset=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale + offset).half().to(DEV)


def last(ops):
    return ops.last_kernel().split(";")[-1]


def gn_silu_ref(x, gamma, beta, eps=1e-5):
    n, h, w, C = x.shape
    g = x.double().reshape(n, h * w, 32, C // 32)
    mu = g.mean(dim=(1, 3), keepdim=True)
    var = ((g - mu) ** 2).mean(dim=(1, 3), keepdim=True)
    xn = ((g - mu) / torch.sqrt(var + eps)).reshape(n, h, w, C) * gamma.double() + beta.double()
    return xn * torch.sigmoid(xn)


def folded_ref(xin, wt, b, s1, s2, wsk, bsk, gn):
    """y_hat and bound of the folded contraction; xin: the fp64 operand of the 3x3 segment (x, or SiLU(GN(x)) when gn)."""
    cout = wt.shape[0]
    sk = (s1 if s2 is None else torch.cat([s1, s2], -1)).double()
    main = EB.im2col(xin, 3)
    wm_main = wt.double().reshape(cout, -1)
    cols = torch.cat([main, sk.reshape(-1, sk.shape[-1])], 1)
    wm = torch.cat([wm_main, wsk.double()], 1)
    extra = (EB.U + 1e-5) * (main.abs() @ wm_main.abs().t()) if gn else None
    return EB.epilogue_ref(cols @ wm.t(), cols.abs() @ wm.abs().t(), wm.shape[1], b.double() + bsk.double(), None, extra=extra)


W64_GN = "conv6_kernel<W64,halo+groupnorm>"

# (n, c, sc1, sc2, expected route): W64, N = 320, out_layers' GroupNorm fused into the halo loader
GN_CASES = [
    (12, 320, 320, 320, W64_GN),                               # 10 slabs, 20 skip steps
    (12, 320, 640, 320, W64_GN),                               # the skip's concat boundary (640) is not the main segment's; 30 skip steps
    (12, 320, 320, 0, W64_GN),                                 # one source, 10 skip steps
    (6, 1024, 320, 0, W64_GN + "+splitk_reduce_kernel"),       # three slices of 10 / 11 / 11 slabs and 3 / 3 / 4 skip steps: both buffer parities
]


@pytest.mark.parametrize("n,c,sc1,sc2,route", GN_CASES, ids=lambda v: str(v))
def test_w64_groupnorm_skip(ops, n, c, sc1, sc2, route):
    """gamma ~ 3, beta ~ -2: a skip chunk normalised by mistake (x * rstd gamma + shift, SiLU) is off by O(|x|) per element, orders above the bound."""
    h = w = 64
    cout, K = 320, 9 * c + sc1 + sc2
    x = r16((n, h, w, c), 71, 1.0, 0.3)
    s1 = r16((n, h, w, sc1), 72, 2.0)
    s2 = r16((n, h, w, sc2), 73, 1.0, -0.5) if sc2 else None
    gamma, beta = r16((c,), 74, 0.2, 3.0), r16((c,), 75, 0.2, -2.0)
    wt = r16((cout, c, 3, 3), 76, 1 / math.sqrt(K))
    wsk = r16((cout, sc1 + sc2), 77, 1 / math.sqrt(K))
    b, bsk = r16((cout,), 78, 0.5), r16((cout,), 79, 0.5)
    y = ops.group_norm_silu_conv2d_skip(x, gamma, beta, 1e-5, ops.repack_conv_weight(wt), b, s1, s2, wsk, bsk)
    assert last(ops) == route
    ref, bound = folded_ref(gn_silu_ref(x, gamma, beta), wt, b, s1, s2, wsk, bsk, gn=True)
    EB.check(y.reshape(-1, cout), ref, bound, f"{route} n{n} c{c} skip {sc1}+{sc2}", image_rows=h * w, width=w, tile=(256, 320))


W16_SPLIT = "conv6_kernel<W16,halo>+splitk_reduce_gn_kernel"


@pytest.mark.parametrize("c", [1280, 1344], ids=lambda v: f"c{v}")
def test_w16_split_skip_with_partials(ops, c):
    """W16, N = 1280, 9 Cin >= 8640: four slices over K (10 slabs each; Cin = 1344: 10 / 11 / 10 / 11), 20 of the 80 skip steps behind each, two
    skip sources, summed in splitk_reduce_gn_kernel.  The partial statistics the reduce writes are those of the returned (folded) tensor."""
    n, h, w, cout, sc1, sc2 = 12, 16, 16, 1280, 1280, 1280
    K = 9 * c + sc1 + sc2
    x, s1, s2 = r16((n, h, w, c), 81), r16((n, h, w, sc1), 82, 2.0), r16((n, h, w, sc2), 83, 1.0, -0.5)
    wt = r16((cout, c, 3, 3), 84, 1 / math.sqrt(K))
    wsk = r16((cout, sc1 + sc2), 85, 1 / math.sqrt(K))
    b, bsk = r16((cout,), 86, 0.5), r16((cout,), 87, 0.5)
    y, part = ops.group_norm_silu_conv2d_skip(x, None, None, 0.0, ops.repack_conv_weight(wt), b, s1, s2, wsk, bsk, partials=True)
    assert last(ops) == W16_SPLIT
    ref, bound = folded_ref(x.double(), wt, b, s1, s2, wsk, bsk, gn=False)
    EB.check(y.reshape(-1, cout), ref, bound, f"{W16_SPLIT} c{c}", image_rows=h * w, width=w, tile=(256, 320))
    assert part is not None
    yg = y.double().view(n, h * w, 32, cout // 32)
    got = part.double().sum(1)
    want = torch.stack([yg.sum((1, 3)), (yg * yg).sum((1, 3))], -1)
    tol = torch.stack([yg.abs().sum((1, 3)), (yg * yg).sum((1, 3))], -1) * (EB.c_acc(h * w * cout // 32) + 2.0 ** -22) + EB.TINY
    assert bool(((got - want).abs() <= tol).all()), float(((got - want).abs() / tol).max())


def test_w16_split_bias_counted_once(ops):
    """Zero weights, non-zero biases (multiples of 2^-6, so that b + bskip is an fp16 number): every element is exactly b + bskip — each
    slice adds none, the reduce pass adds it once."""
    n, h, w, c, cout, sc1, sc2 = 12, 16, 16, 1280, 1280, 1280, 1280
    x, s1, s2 = r16((n, h, w, c), 91), r16((n, h, w, sc1), 92), r16((n, h, w, sc2), 93)
    wt = torch.zeros(cout, c, 3, 3, dtype=torch.float16, device=DEV)
    wsk = torch.zeros(cout, sc1 + sc2, dtype=torch.float16, device=DEV)
    g = torch.Generator().manual_seed(94)
    b = (torch.randint(-96, 97, (cout,), generator=g).float() / 64).half().to(DEV)
    bsk = (torch.randint(-96, 97, (cout,), generator=g).float() / 64).half().to(DEV)
    y = ops.conv2d_skip(x, ops.repack_conv_weight(wt), b, s1, s2, wsk, bsk)
    assert last(ops) == "conv6_kernel<W16,halo>+splitk_reduce_kernel"
    want = (b.double() + bsk.double()).half()
    assert bool((y.reshape(-1, cout) == want).all())


def test_w32_skip(ops):
    """W32 at N = 640 (no GroupNorm fusion: the output is two tiles wide), one skip source of 320 channels: input_blocks.4's shape."""
    n, h, w, c, cout, sc1 = 24, 32, 32, 640, 640, 320
    route = "conv6_kernel<W32,halo>"
    K = 9 * c + sc1
    x, s1 = r16((n, h, w, c), 101), r16((n, h, w, sc1), 102, 2.0)
    wt = r16((cout, c, 3, 3), 103, 1 / math.sqrt(K))
    wsk = r16((cout, sc1), 104, 1 / math.sqrt(K))
    b, bsk = r16((cout,), 105, 0.5), r16((cout,), 106, 0.5)
    y = ops.conv2d_skip(x, ops.repack_conv_weight(wt), b, s1, None, wsk, bsk)
    assert last(ops) == route
    ref, bound = folded_ref(x.double(), wt, b, s1, None, wsk, bsk, gn=False)
    EB.check(y.reshape(-1, cout), ref, bound, route, image_rows=h * w, width=w, tile=(256, 320))


@pytest.mark.parametrize("hw,n,c,cout,sc1,sc2,bias,gn,route", [
    (64, 12, 320, 320, 320, 320, 1.5, True, W64_GN),
    (16, 12, 1280, 1280, 1280, 1280, 2.0, False, "conv6_kernel<W16,halo>+splitk_reduce_kernel"),
], ids=["W64", "W16"])
def test_border_exactness(ops, hw, n, c, cout, sc1, sc2, bias, gn, route):
    """All-ones inputs, skip weights of ones, main weights zero: every element — the first and last row and column of every image included —
    is exactly sc1 + sc2 + b + bskip (643 and 2564: fp16 numbers).  A border or zero-page rule leaking into the centre-only image would
    lose whole channels at the image edges."""
    ones = lambda *s: torch.ones(*s, dtype=torch.float16, device=DEV)
    x, s1, s2 = ones(n, hw, hw, c), ones(n, hw, hw, sc1), ones(n, hw, hw, sc2)
    wt = torch.zeros(cout, c, 3, 3, dtype=torch.float16, device=DEV)
    b, bsk = ones(cout) * bias, ones(cout) * bias
    gamma, beta = (ones(c) * 3.0, ones(c) * -2.0) if gn else (None, None)
    y = ops.group_norm_silu_conv2d_skip(x, gamma, beta, 1e-5, ops.repack_conv_weight(wt), b, s1, s2, ones(cout, sc1 + sc2), bsk)
    assert last(ops) == route
    assert bool((y == float(sc1 + sc2) + 2 * bias).all()), (float(y.min()), float(y.max()))
