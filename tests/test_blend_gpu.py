"""GPU: tiled_scale's accumulation and final divide (tile_blend_kernel, tile_divide_kernel of esrgan.hip, through upscale.blend_tile), held
element-wise against the fp64 accumulation of the same tiles in the same order (tests/errbound.py tile_blend_ref): the blended canvas, the `div`
plane and the quotient.  Overlapping tiles, one flush with the far corner, one of 17 x 19 pixels (not a multiple of a block), a one-row canvas,
one and three channels; canvas bytes outside a tile stay as they were bit for bit; a tile that leaves the canvas is refused.

KERNELS names, per kernel, the tests that hold it (tests/test_errbound_cpu.py keeps the ledger)."""
import pytest
import torch

import errbound as EB
from lightdiffusion_amd._lib import ERR_ARG, ERR_SHAPE, OK

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

KERNELS = {
    "tile_blend_kernel": ["test_tile_blend", "test_tile_blend_leaves_the_rest_alone", "test_tile_blend_rejects"],
    "tile_divide_kernel": ["test_tile_blend"],
}

# canvas (oh, ow) -> tiles (y0, x0, th, tw), accumulated in this order: four overlapping quarters (the last flush with the far corner), a
# 17 x 19 tile flush with the far corner and one inside
CANVASES = {
    (40, 56): [(0, 0, 24, 32), (0, 24, 24, 32), (16, 0, 24, 32), (16, 24, 24, 32), (23, 37, 17, 19), (5, 9, 17, 19)],
    (1, 300): [(0, 0, 1, 200), (0, 100, 1, 200), (0, 281, 1, 19)],
}


def make_tiles(rects, c, seed):
    g = torch.Generator().manual_seed(seed)
    ramp = lambda n: torch.minimum(torch.arange(1, n + 1), torch.arange(n, 0, -1)).float().clamp_max(4) / 4.0 * (0.5 + torch.rand(1, generator=g))
    return [(torch.randn(th, tw, c, generator=g), ramp(th), ramp(tw), y0, x0) for (y0, x0, th, tw) in rects]


def held(y, ref, bound, what):
    r, s = EB.check(y, ref, bound, what, keep=torch.ones_like(ref, dtype=torch.bool), bias_extra=EB.rtn_noise(ref.numel()))
    print(f"{what}: error / bound {r:.3f}, signed bias {s:+.2e}")


@pytest.mark.parametrize("c", [3, 1])
@pytest.mark.parametrize("canvas", list(CANVASES), ids=lambda v: f"{v[0]}x{v[1]}")
def test_tile_blend(canvas, c):
    from lightdiffusion_amd.upscale import blend_tile
    oh, ow = canvas
    tiles = make_tiles(CANVASES[canvas], c, 10 * oh + c)
    out = torch.zeros(oh, ow, c, device=DEV)
    div = torch.zeros(oh, ow, device=DEV)
    for ps, my, mx, y0, x0 in tiles:
        blend_tile(ps.to(DEV), my.to(DEV), mx.to(DEV), out, div, y0, x0)
    r_out, b_out, r_div, b_div, r_quot, b_quot = EB.tile_blend_ref(oh, ow, c, tiles)
    assert float(r_div.min()) > 0.0                       # every pixel is covered: the quotient is defined
    what = f"tile_blend {oh}x{ow} c={c}"
    held(out.cpu(), r_out, b_out, what + " out")
    held(div.cpu(), r_div, b_div, what + " div")
    # the divide against the quotient of the DEVICE's accumulated planes: one fp32 ulp, and against the fp64 quotient: the carried bound
    acc, plane = out.cpu().double(), div.cpu().double()
    blend_tile(None, None, None, out, div)
    q = acc / plane.unsqueeze(-1)
    held(out.cpu(), q, 2.0 ** -23 * q.abs() + 1e-30, what + " divide")
    held(out.cpu(), r_quot, b_quot, what + " quotient")
    assert torch.equal(div.cpu().double(), plane)         # the divide leaves div alone


def test_tile_blend_leaves_the_rest_alone():
    """One 17 x 19 tile on a canvas of NaN-free random bits: everything outside the tile is unchanged bit for bit, inside it is out0 + ps m."""
    from lightdiffusion_amd.upscale import blend_tile
    g = torch.Generator().manual_seed(4)
    oh, ow, c = 40, 56, 3
    out0, div0 = torch.randn(oh, ow, c, generator=g), torch.rand(oh, ow, generator=g) + 0.5
    (tile,) = make_tiles([(23, 37, 17, 19)], c, 5)
    out, div = out0.to(DEV), div0.to(DEV)
    blend_tile(tile[0].to(DEV), tile[1].to(DEV), tile[2].to(DEV), out, div, 23, 37)
    outside = torch.ones(oh, ow, dtype=torch.bool)
    outside[23:40, 37:56] = False
    assert torch.equal(out.cpu()[outside].view(torch.int32), out0[outside].view(torch.int32))
    assert torch.equal(div.cpu()[outside].view(torch.int32), div0[outside].view(torch.int32))
    r_out, b_out, r_div, b_div, _, _ = EB.tile_blend_ref(oh, ow, c, [tile], out0, div0)
    held(out.cpu(), r_out, b_out, "tile_blend onto a filled canvas, out")
    held(div.cpu(), r_div, b_div, "tile_blend onto a filled canvas, div")


def test_tile_blend_rejects():
    from lightdiffusion_amd._lib import lib
    l, s = lib(), torch.cuda.current_stream().cuda_stream
    out, div = torch.zeros(8, 8, 3, device=DEV), torch.zeros(8, 8, device=DEV)
    ps, my, mx = torch.ones(4, 4, 3, device=DEV), torch.ones(4, device=DEV), torch.ones(4, device=DEV)
    p = lambda t: t.data_ptr()
    call = lambda y0, x0, th=4, tw=4: l.ld_op_tile_blend(p(ps), p(my), p(mx), th, tw, p(out), p(div), 8, 8, y0, x0, 3, s)
    for y0, x0 in ((5, 0), (0, 5), (-1, 0), (0, -1), (8, 8)):
        assert call(y0, x0) == ERR_SHAPE, (y0, x0)
    assert l.ld_op_tile_blend(p(ps), None, p(mx), 4, 4, p(out), p(div), 8, 8, 0, 0, 3, s) == ERR_ARG
    assert l.ld_op_tile_blend(p(ps), p(my), p(mx), 4, 4, None, p(div), 8, 8, 0, 0, 3, s) == ERR_ARG
    torch.cuda.synchronize()
    assert bool((out == 0).all()) and bool((div == 0).all())
    assert call(4, 4) == OK                               # flush with the far corner is inside
    torch.cuda.synchronize()
    assert bool((out[4:, 4:] == 1).all()) and bool((out[:4] == 0).all()) and bool((div[4:, 4:] == 1).all())
