"""GPU: regional conditioning's two fp32 kernels (csrc/regional/regional.hip) through lightdiffusion_amd.ops.
  gather    BITWISE against slicing + cat;
  combine   BITWISE against tests/regional_ref.py — upstream's get_area_and_mult and calc_cond_batch loops restated operation by operation in
            torch fp32 on the host (IEEE products, sums and divisions are the same bits on either side; the unit is built without contraction).
No tolerance anywhere.  Latents: 16 x 24 (W and every window's x0 and w multiples of 4: the float4 path), 17 x 23 with odd window offsets (the
scalar path), 8 x 8 with whole-latent areas only (no feather at all); B in {1, 2}, C = 4.  Entry sets: a lone whole entry per list; two areas that
overlap inside both of their ramps; an area that touches two edges of the latent (no ramp there); masks of 0 / 1 and of fractions with Bm = 1 and
Bm = B; a pixel that no cond entry covers; 16 entries.  Inputs are seeded randn; mask values, strengths and mask strengths are multiples of 1/64
with few bits, so no product is subnormal.
KERNELS names the tests that hold each kernel; tests/test_regional_ledger_cpu.py keeps that ledger."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import regional_ref as R                                       # noqa: E402
from lightdiffusion_amd import ops                             # noqa: E402
from lightdiffusion_amd._lib import ERR_ARG, ERR_SHAPE, OK, RegionalEntry, RegionalWindow, lib     # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E = ops.RegionalEntry
same_bits = R.same_bits

KERNELS = {
    "regional_gather_kernel": ("test_gather", "test_unaligned_pointers_take_the_scalar_path", "test_launches_are_capturable"),
    "regional_combine_kernel": ("test_combine", "test_combine_uncovered_pixels_give_zero", "test_unaligned_pointers_take_the_scalar_path",
                                "test_launches_are_capturable"),
}

LATENTS = {"vector": (16, 24), "scalar": (17, 23), "whole": (8, 8)}


def mask_of(g, bm, H, W, binary=False):
    m = torch.randint(0, 2, (bm, H, W), generator=g).float() if binary else torch.randint(0, 65, (bm, H, W), generator=g).float() / 64.0
    return m.contiguous()


def entry_sets(kind, B, g):
    """{name: [(list, area (h, w, y0, x0), strength, mask, mask_strength), ...]} in accumulation order, for the latent of `kind`"""
    H, W = LATENTS[kind]
    whole = (H, W, 0, 0)
    sets = {"lone": [(0, whole, 1.0, None, 1.0), (1, whole, 1.0, None, 1.0)]}
    if kind == "whole":
        sets["masks"] = [(1, whole, 1.0, None, 1.0), (0, whole, 0.5, mask_of(g, 1, H, W), 0.75), (0, whole, 1.0, mask_of(g, B, H, W, True), 1.0)]
        return sets
    if kind == "vector":
        a1, a2 = (12, 12, 0, 4), (12, 16, 4, 8)            # overlap rows 4..11, columns 8..15: inside a1's bottom / right and a2's top / left ramps
        corner, small = (8, 8, 8, 16), (8, 8, 4, 4)        # corner touches the bottom and the right edge of the latent
        spread = lambda i: (8 + 4 * (i % 2), 8 + 4 * (i % 3), (i * 3) % 5, 4 * ((i // 3) % 3))
    else:
        a1, a2 = (11, 13, 1, 3), (10, 12, 5, 9)            # odd offsets; overlap rows 5..11, columns 9..15
        corner, small = (9, 11, 8, 12), (8, 9, 3, 5)       # 8 + 9 = 17, 12 + 11 = 23
        spread = lambda i: (8 + (i % 5), 8 + (i % 7), i % 4, (i * 2 + 1) % 7)
    sets["overlap"] = [(1, whole, 1.0, None, 1.0), (0, a1, 1.0, None, 1.0), (0, a2, 0.75, None, 1.0), (1, a2, 1.25, None, 1.0)]
    sets["corner"] = [(0, whole, 1.0, None, 1.0), (0, corner, 1.5, None, 1.0), (1, corner, 1.0, None, 1.0), (1, whole, 0.5, None, 1.0)]
    sets["masks"] = [(1, whole, 1.0, None, 1.0), (0, whole, 1.0, mask_of(g, 1, H, W, True), 1.0), (0, whole, 0.5, mask_of(g, B, H, W), 0.75),
                     (0, a1, 1.0, mask_of(g, B, H, W), 1.0), (1, a2, 1.0, mask_of(g, 1, H, W), 0.5)]
    sets["uncovered"] = [(0, small, 1.0, None, 1.0), (1, whole, 1.0, None, 1.0)]
    sets["sixteen"] = [(i % 2, spread(i), 1.0 + (i % 3) / 4.0, mask_of(g, 1 if i % 4 else B, H, W) if i % 5 == 0 else None, 0.5 + (i % 2) / 2.0)
                       for i in range(16)]
    return sets


CASES = [(kind, name) for kind in LATENTS for name in (("lone", "masks") if kind == "whole" else ("lone", "overlap", "corner", "masks", "uncovered", "sixteen"))]


def build(kind, name, B, C=4, seed=0):
    """-> (outs, entries, shape) on the host: the entries grouped by area shape as the sampler groups them, outs seeded randn"""
    g = torch.Generator().manual_seed(1000 * seed + 17 * B + len(name))
    H, W = LATENTS[kind]
    rows = entry_sets(kind, B, g)[name]
    shapes = []
    for _, a, _, _, _ in rows:
        if a[:2] not in shapes:
            shapes.append(a[:2])
    slots = {s: 0 for s in shapes}
    entries = []
    for l, a, st, m, ms in rows:
        entries.append(E(l, shapes.index(a[:2]), slots[a[:2]], a, st, m, ms))
        slots[a[:2]] += 1
    outs = [torch.randn(slots[s] * B, C, s[0], s[1], generator=g) * 3.0 for s in shapes]
    return outs, entries, (B, C, H, W)


def to_dev(outs, entries):
    return [o.to(DEV) for o in outs], [e._replace(mask=None if e.mask is None else e.mask.to(DEV)) for e in entries]


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("kind", list(LATENTS))
def test_gather(kind, B):
    H, W = LATENTS[kind]
    g = torch.Generator().manual_seed(B)
    x = torch.randn(B, 4, H, W, generator=g)
    dx = x.to(DEV)
    groups = {"vector": [[(8, 16, 0, 4), (8, 16, 8, 8), (8, 16, 4, 0)], [(12, 10, 1, 3)]],     # the second has a width that is no multiple of 4
              "scalar": [[(9, 11, 3, 5), (9, 11, 8, 12), (9, 11, 0, 0)], [(8, 8, 1, 1)]],
              "whole": [[(8, 8, 0, 0)]]}[kind]
    groups.append([(H, W, 0, 0)] * 3)                                                          # a whole-latent group: the latent three times
    groups.append([(8, 8, i % (H - 7), (2 * i) % (W - 7)) for i in range(16)])
    for windows in groups:
        got = ops.regional_gather(dx, windows)
        assert got.is_contiguous() and tuple(got.shape) == (len(windows) * B, 4) + windows[0][:2]
        assert same_bits(got.cpu(), R.gather(x, windows)), windows
    assert same_bits(dx.cpu(), x), "the latent is read only"
    out = torch.full((2 * B, 4, 8, 8), -7.0, device=DEV)
    assert ops.regional_gather(dx, [(8, 8, 0, 0)] * 2, out=out) is out and same_bits(out.cpu(), torch.cat([x[:, :, :8, :8]] * 2))


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("kind,name", CASES)
def test_combine(kind, name, B):
    outs, entries, shape = build(kind, name, B)
    douts, dentries = to_dev(outs, entries)
    got = ops.regional_combine(douts, dentries, 7.5, shape)
    assert got.is_contiguous() and tuple(got.shape) == shape and got.device.type == "cuda"
    want = R.combine(outs, entries, 7.5, shape)
    assert torch.isfinite(want).all()
    assert same_bits(got.cpu(), want)
    assert same_bits(ops.regional_combine(outs, entries, 7.5, shape), want), "and the ops' host branch is the same expression"
    for before, after in zip(outs, douts):
        assert same_bits(after.cpu(), before), "the inputs are read only"
    if name == "sixteen":
        assert len(entries) == 16 and len(outs) > 4


def test_combine_lone_entries_are_the_cfg_mix():
    """one whole unkeyed entry per list: out * 1 / (1e-37 + 1) is out, and the result is u + (c - u) * scale"""
    outs, entries, shape = build("vector", "lone", 2, seed=3)
    got = ops.regional_combine(*to_dev(outs, entries), 3.0, shape).cpu()
    c, u = outs[0][:2], outs[0][2:]
    assert same_bits(got, u + (c - u) * 3.0)


@pytest.mark.parametrize("kind", ["vector", "scalar"])
def test_combine_uncovered_pixels_give_zero(kind):
    """where no cond entry covers a pixel the cond prediction is 0 / 1e-37 = 0: the result there is u + (0 - u) * scale"""
    outs, entries, shape = build(kind, "uncovered", 2, seed=4)
    got = ops.regional_combine(*to_dev(outs, entries), 7.5, shape).cpu()
    h, w, y0, x0 = entries[0].area
    u = outs[entries[1].group][entries[1].slot * 2:entries[1].slot * 2 + 2]
    outside = torch.ones(shape, dtype=torch.bool)
    outside[:, :, y0:y0 + h, x0:x0 + w] = False
    assert same_bits(got[outside], (u + (0.0 - u) * 7.5)[outside])
    assert not torch.equal(got[~outside], (u + (0.0 - u) * 7.5)[~outside])


def raw_tables(douts, dentries, B, C, offset=0, like=None):
    """the ABI's entry table for device tensors (`like`: the entries whose masks have the true shapes, where dentries' are flat buffers)"""
    tab = (RegionalEntry * len(dentries))()
    for t, e, o in zip(tab, dentries, like or dentries):
        h, w, y0, x0 = e.area
        t.out = douts[e.group].data_ptr() + offset + e.slot * B * C * h * w * 4
        t.mask = None if e.mask is None else e.mask.data_ptr() + offset
        t.list, t.mask_batch, t.y0, t.x0, t.h, t.w = e.list, 1 if o.mask is None else o.mask.shape[0], y0, x0, h, w
        t.strength, t.mask_strength = e.strength, e.mask_strength
    return tab


def test_unaligned_pointers_take_the_scalar_path():
    """16 x 24 latents whose buffers start 4 bytes off a 16-byte boundary (views into larger buffers, handed to the raw entries): the float4
    path is for aligned pointers only, and the result is the same bits; nothing outside the tensors is written."""
    B, C = 2, 4
    outs, entries, shape = build("vector", "masks", B, seed=5)
    stream = torch.cuda.current_stream().cuda_stream

    def off_by_one(t):
        buf = torch.zeros(t.numel() + 4, device=DEV)
        buf[1:1 + t.numel()] = t.flatten().to(DEV)
        return buf
    bouts = [off_by_one(o) for o in outs]
    bmasks = [None if e.mask is None else off_by_one(e.mask) for e in entries]
    shifted = [e._replace(mask=bm) for e, bm in zip(entries, bmasks)]
    n = B * C * 16 * 24
    res = torch.full((n + 4,), -7.0, device=DEV)
    tab = raw_tables(bouts, shifted, B, C, offset=4, like=entries)
    assert tab[0].out % 16 == 4
    assert lib().ld_op_regional_combine(tab, len(tab), 7.5, res.data_ptr() + 4, B, C, 16, 24, stream) == OK
    assert same_bits(res[1:1 + n].view(shape).cpu(), R.combine(outs, entries, 7.5, shape))
    assert res[0].item() == -7.0 and bool((res[1 + n:] == -7.0).all()), "nothing outside the tensor is written"
    x = torch.randn(shape, generator=torch.Generator().manual_seed(6))
    bx = off_by_one(x)
    windows = [(8, 16, 0, 4), (8, 16, 8, 8)]
    m = 2 * B * C * 8 * 16
    out = torch.full((m + 4,), -7.0, device=DEV)
    wtab = (RegionalWindow * 2)(*[RegionalWindow(y0, x0) for _, _, y0, x0 in windows])
    assert lib().ld_op_regional_gather(bx.data_ptr() + 4, out.data_ptr() + 4, B, C, 16, 24, 8, 16, wtab, 2, stream) == OK
    assert same_bits(out[1:1 + m].view(2 * B, C, 8, 16).cpu(), R.gather(x, windows))
    assert out[0].item() == -7.0 and bool((out[1 + m:] == -7.0).all())


def test_launches_are_capturable():
    """Stream-ordered, no allocation with `out` given, no host read: both launches go into a hipGraph; the descriptors were copied into the
    kernel arguments at capture, and a replay reads what is in device memory then."""
    B = 2
    outs, entries, shape = build("vector", "overlap", B, seed=7)
    douts, dentries = to_dev(outs, entries)
    x = torch.randn(shape, generator=torch.Generator().manual_seed(8))
    dx = x.to(DEV)
    windows = [(12, 16, 4, 8), (12, 16, 0, 4)]
    gat = torch.zeros(2 * B, 4, 12, 16, device=DEV)
    res = torch.zeros(shape, device=DEV)
    ops.regional_gather(dx, windows, out=gat)                  # warm-up outside capture
    ops.regional_combine(douts, dentries, 7.5, shape, out=res)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        ops.regional_gather(dx, windows, out=gat)
        ops.regional_combine(douts, dentries, 7.5, shape, out=res)
    gen = torch.Generator().manual_seed(9)
    x2 = torch.randn(shape, generator=gen)
    outs2 = [torch.randn(o.shape, generator=gen) for o in outs]
    dx.copy_(x2)
    for d, o in zip(douts, outs2):
        d.copy_(o)
    gat.zero_()
    res.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert same_bits(gat.cpu(), R.gather(x2, windows))
    assert same_bits(res.cpu(), R.combine(outs2, entries, 7.5, shape))


def test_rejections():
    B, C, H, W = 2, 4, 16, 24
    outs, entries, shape = build("vector", "overlap", B, seed=10)
    douts, dentries = to_dev(outs, entries)
    dx = torch.randn(shape, device=DEV)
    res = torch.full(shape, -7.0, device=DEV)
    gat = torch.full((B, C, 8, 8), -7.0, device=DEV)
    one = (RegionalWindow * 1)(RegionalWindow(0, 0))
    gather = lambda px, po, tab=one, B=B, C=C, H=H, W=W, h=8, w=8, k=1: lib().ld_op_regional_gather(px, po, B, C, H, W, h, w, tab, k, None)
    assert gather(None, gat.data_ptr()) == ERR_ARG and gather(dx.data_ptr(), None) == ERR_ARG and gather(dx.data_ptr(), gat.data_ptr(), tab=None) == ERR_ARG
    p = (dx.data_ptr(), gat.data_ptr())
    for bad in (dict(B=0), dict(C=0), dict(H=0), dict(W=-1), dict(h=0), dict(w=0), dict(h=17), dict(w=25), dict(k=0), dict(k=17),
                dict(B=1 << 15, C=1 << 15, H=2, W=1, h=1, w=1)):                     # 2^31 floats: the kernels index in 32 bits
        assert gather(*p, **bad) == ERR_SHAPE, bad
    for y0, x0 in ((-1, 0), (0, -1), (9, 0), (0, 17)):                              # a window that leaves the latent
        assert gather(*p, tab=(RegionalWindow * 1)(RegionalWindow(y0, x0))) == ERR_SHAPE, (y0, x0)
    tab = raw_tables(douts, dentries, B, C)
    combine = lambda t=tab, n=len(tab), pr=res.data_ptr(), B=B, C=C, H=H, W=W: lib().ld_op_regional_combine(t, n, 7.5, pr, B, C, H, W, None)
    assert combine(t=None) == ERR_ARG and combine(pr=None) == ERR_ARG
    nul = raw_tables(douts, dentries, B, C)
    nul[1].out = None
    assert combine(t=nul) == ERR_ARG
    for bad in (dict(n=0), dict(n=17), dict(B=0), dict(C=0), dict(H=0), dict(W=0), dict(H=15), dict(W=20), dict(B=1 << 15, C=1 << 15)):
        assert combine(**bad) == ERR_SHAPE, bad
    for field, value in (("list", 2), ("h", 0), ("w", -4), ("y0", -1), ("x0", 12), ("y0", 8)):
        t = raw_tables(douts, dentries, B, C)
        setattr(t[2], field, value)
        assert combine(t=t) == ERR_SHAPE, (field, value)
    t = raw_tables(*to_dev(*build("vector", "masks", B, seed=10)[:2]), B, C)
    t[1].mask_batch = 3
    assert combine(t=t, n=len(t)) == ERR_SHAPE
    torch.cuda.synchronize()
    assert bool((res == -7.0).all()) and bool((gat == -7.0).all()), "a refused call launches nothing"
    with pytest.raises(ValueError, match="leaves the"):
        ops.regional_gather(dx, [(8, 8, 9, 0)])
    with pytest.raises(ValueError, match="one shape"):
        ops.regional_gather(dx, [(8, 8, 0, 0), (8, 12, 0, 0)])
    with pytest.raises(ValueError, match="windows"):
        ops.regional_gather(dx, [(8, 8, 0, 0)] * 17)
    with pytest.raises(ValueError, match="dtype"):
        ops.regional_gather(dx.half(), [(8, 8, 0, 0)])
    with pytest.raises(ValueError, match="contiguous"):
        ops.regional_gather(dx.permute(0, 1, 3, 2), [(8, 8, 0, 0)])
    with pytest.raises(ValueError, match="entries"):
        ops.regional_combine(douts, dentries * 5, 7.5, shape)
    with pytest.raises(ValueError, match="side < 1"):
        ops.regional_combine(douts, [dentries[0]._replace(area=(0, 24, 0, 0))] + dentries[1:], 7.5, shape)
    with pytest.raises(ValueError, match="do not fit"):
        ops.regional_combine(douts, [dentries[0]._replace(slot=1)] + dentries[1:], 7.5, shape)
    with pytest.raises(ValueError, match="list"):
        ops.regional_combine(douts, [dentries[0]._replace(list=2)] + dentries[1:], 7.5, shape)
    with pytest.raises(ValueError, match="mask"):
        ops.regional_combine(douts, [dentries[0]._replace(mask=torch.ones(3, H, W, device=DEV))] + dentries[1:], 7.5, shape)
    with pytest.raises(ValueError, match="mask"):
        ops.regional_combine(douts, [dentries[0]._replace(mask=torch.ones(1, H, W))] + dentries[1:], 7.5, shape)          # a mask on the host
    with pytest.raises(ValueError, match="2\\^31"):
        ops.regional_combine(douts, dentries, 7.5, (1 << 15, 1 << 15, 2, 1))
    assert gather(*p) == OK and combine() == OK
    torch.cuda.synchronize()
