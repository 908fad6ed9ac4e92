"""GPU: every kernel of norm.hip held element-wise (tests/errbound.py) against an fp64 reference from the same fp16 inputs, at the channel
layouts, pixel-chunk geometries and statistics where the kernels take another path.  Each case prints its worst error / bound and signed bias.

KERNELS names, per kernel, the tests that hold it (tests/test_errbound_cpu.py checks that no kernel of norm.hip is missing)."""
import pytest
import torch

import errbound as EB
from lightdiffusion_amd._lib import ERR_SHAPE, LDError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

KERNELS = {
    "gn_stats_kernel": ["test_groupnorm_layouts", "test_groupnorm_pixel_geometry", "test_groupnorm_partials_are_the_chunk_sums"],
    "gn_apply_kernel": ["test_groupnorm_layouts", "test_groupnorm_pixel_geometry", "test_groupnorm_statistics_under_stress", "test_groupnorm_from_partials"],
    "gn_finalize_kernel": ["test_groupnorm_scale_shift_is_what_apply_uses", "test_groupnorm_from_partials"],
    "layernorm_kernel": ["test_layernorm"],
    "softmax_rows_kernel": ["test_softmax_rows"],
}


@pytest.fixture(scope="module")
def ops():
    from lightdiffusion_amd import ops as o
    from lightdiffusion_amd._lib import lib
    lib()
    return o


def held(y, ref, bound, what, keep=None, bias_extra=0.0):
    """EB.check on every element; the bias statistic's floor must keep at least half of them (its tolerance: BIAS_TOL + the chance level
    of that many independent round-to-nearest errors, EB.rtn_noise)."""
    if keep is None:
        frac = EB.bias_kept_fraction(ref)
        assert frac >= 0.5, f"{what}: the bias statistic keeps only {frac:.2f} of the elements"
    r, s = EB.check(y, ref, bound, what, keep=keep, bias_extra=bias_extra + EB.rtn_noise(EB.independent_roundings(ref, keep)))
    print(f"{what}: error / bound {r:.3f}, signed bias {s:+.2e}")
    return r, s


# ------------------------------------------------------------------ GroupNorm
def gn_input(n, hw, c1, c2, seed, offsets=None, scales=None):
    """x [n][hw][C] with a different mean and scale for each of the 32 groups (statistics leaking between groups show), split at c1."""
    c = c1 + c2
    g = torch.Generator().manual_seed(seed)
    grp = torch.arange(c) // (c // 32)
    off = (grp.float() - 15.5) * 0.25 if offsets is None else offsets[grp]
    sc = 0.5 + (grp % 5).float() * 0.3 if scales is None else scales[grp]
    x = (torch.randn(n, hw, c, generator=g) * sc + off).half().to(DEV)
    ga = (1.0 + 0.5 * torch.randn(c, generator=g)).half().to(DEV)
    be = (0.5 * torch.randn(c, generator=g)).half().to(DEV)
    x1 = x[..., :c1].contiguous()
    x2 = x[..., c1:].contiguous() if c2 else None
    return x1, x2, ga, be


def gn_case(ops, n, hw, c1, c2, seed, eps, silu, **kw):
    x1, x2, ga, be = gn_input(n, hw, c1, c2, seed, **kw)
    y = ops.group_norm(x1, ga, be, eps, silu, x2)
    ref, bound = EB.groupnorm_ref(x1, x2, ga, be, eps, silu)
    held(y.reshape(ref.shape), ref, bound, f"groupnorm n={n} hw={hw} C={c1}+{c2} eps={eps} silu={silu}")
    return x1, x2, ga, be, y


# (c1, c2, n, hw): one slab C < 128 (C = 96: cpg = 3, an 8-channel chunk spans three groups), two slabs C < 256, four from 256 (C = 320: cpg = 10, 25 pixel
# rows and 6 idle threads), the largest C, and concatenations whose boundary lies inside a group (8 + 24), on a group edge (64 + 32), off a slab edge (320 + 640)
LAYOUTS = [(32, 0, 2, 40), (64, 0, 2, 40), (96, 0, 2, 40), (128, 0, 2, 40), (192, 0, 2, 40), (256, 0, 2, 40), (320, 0, 2, 40), (8192, 0, 1, 8),
           (8, 24, 2, 35), (64, 32, 2, 35), (320, 640, 2, 35), (1280, 1280, 1, 64)]


@pytest.mark.parametrize("c1,c2,n,hw", LAYOUTS)
def test_groupnorm_layouts(ops, c1, c2, n, hw):
    for i, (eps, silu) in enumerate([(1e-5, False), (1e-5, True), (1e-6, False), (1e-6, True)]):
        gn_case(ops, n, hw, c1, c2, 100 + i, eps, silu)


def test_groupnorm_rejects_more_than_8192_channels(ops):
    x1, _, ga, be = gn_input(1, 8, 8224, 0, 3)
    with pytest.raises(LDError) as e:
        ops.group_norm(x1, ga, be, 1e-5)
    assert e.value.status == ERR_SHAPE


# (n, hw, C) against gn_num_chunks: one pixel; fewer than 8; exactly 8; an EMPTY last chunk (hw = 81, n = 1: P = 10, ppb = 9, chunk 9 starts at pixel 81);
# hw = 77 at n = 3; C = 2048 (rows_par = 4) at n = 8 with ppb = 15 / 16 / 17 — the 4-pixel unrolled loop with a tail in some rows, without a tail, and
# with one tail pixel; hw = 16384 at n = 1 (P at its cap of 256, ppb = 64)
GEOMETRY = [(1, 1, 64), (1, 7, 64), (1, 8, 320), (1, 81, 64), (1, 81, 320), (3, 77, 96), (3, 77, 320), (8, 240, 2048), (8, 256, 2048), (8, 272, 2048),
            (1, 16384, 128)]


@pytest.mark.parametrize("n,hw,c", GEOMETRY)
def test_groupnorm_pixel_geometry(ops, n, hw, c):
    from lightdiffusion_amd._lib import lib
    p = lib().ld_op_groupnorm_chunks(n, hw)
    print(f"n={n} hw={hw}: P={p} ppb={(hw + p - 1) // p}")
    if (n, hw) == (1, 81):
        assert p == 10 and (hw + p - 1) // p == 9
    if c == 2048:
        assert p == 16 and (hw + p - 1) // p == hw // 16
    if hw == 16384:
        assert p == 256
    for i, (eps, silu) in enumerate([(1e-5, True), (1e-6, False)]):
        gn_case(ops, n, hw, c, 0, 200 + i, eps, silu)


def test_groupnorm_partials_are_the_chunk_sums(ops):
    """gn_stats_kernel alone: every (image, chunk, group) partial against the fp64 sums of that chunk's pixels, an empty chunk included."""
    for n, hw, c in ((1, 81, 64), (3, 77, 320), (2, 40, 128)):
        x1, _, _, _ = gn_input(n, hw, c, 0, 7)
        part = ops.group_norm_stats(x1)
        p = part.shape[1]
        ppb = (hw + p - 1) // p
        xg = x1.double().reshape(n, hw, 32, c // 32)
        ref = torch.zeros(n, p, 32, 2, dtype=torch.float64, device=DEV)
        mag = torch.zeros_like(ref)
        for k in range(p):
            sl = xg[:, k * ppb:min(hw, (k + 1) * ppb)]
            ref[:, k, :, 0], ref[:, k, :, 1] = sl.sum(dim=(1, 3)), (sl * sl).sum(dim=(1, 3))
            mag[:, k, :, 0], mag[:, k, :, 1] = sl.abs().sum(dim=(1, 3)), (sl * sl).sum(dim=(1, 3))
        bound = EB.c_acc(ppb * (c // 32)) * mag + 1e-30
        held(part, ref, bound, f"gn partials n={n} hw={hw} C={c}", keep=torch.ones_like(ref, dtype=torch.bool))
        if (n, hw) == (1, 81):
            assert bool((part[:, 9] == 0).all()), "the empty last chunk must hold zeros"


def test_groupnorm_statistics_under_stress(ops):
    """Groups with mu / sigma ~ 30 (the cancellation in var = msq - mu^2) and one constant group (var clamped at 0, rstd = eps^-1/2) stay inside the
    derived bound; the print shows how much of the bound the cancellation term is."""
    for c, eps, silu in ((64, 1e-5, False), (320, 1e-6, True), (128, 1e-5, True)):
        off = (torch.arange(32).float() - 15.5) * 0.25
        sc = torch.ones(32)
        off[[3, 17, 30]] = torch.tensor([30.0, -30.0, 15.0])
        sc[30] = 0.5
        off[9], sc[9] = 2.75, 0.0                                   # the constant group
        x1, x2, ga, be = gn_input(2, 77, c, 0, 11, offsets=off, scales=sc)
        y = ops.group_norm(x1, ga, be, eps, silu)
        ref, bound, share = EB.groupnorm_ref(x1, None, ga, be, eps, silu, parts=True)
        cpg = c // 32
        for g in (3, 9, 17, 30, 0):
            sl = slice(g * cpg, (g + 1) * cpg)
            err = (y.double().reshape(ref.shape) - ref)[..., sl].abs()
            print(f"C={c} group {g}: worst error / bound {float((err / bound[..., sl]).max()):.3f}, cancellation term = "
                  f"{float(share[..., sl].max()):.2%} of the bound at most")
        held(y.reshape(ref.shape), ref, bound, f"groupnorm stress C={c} eps={eps} silu={silu}")


def _fma_or_mul_add(x, sc, sh):
    """The two fp32 evaluations of x * sc + sh a compiler may emit, rounded to fp16: fused (one rounding; through fp64, where the product of an
    fp16 and an fp32 number is exact) and unfused."""
    xs = x.float()
    fused = (xs.double() * sc.double() + sh.double()).float().half()
    unfused = (xs * sc + sh).half()
    return fused, unfused


@pytest.mark.parametrize("c1,c2,n,hw", [(64, 0, 2, 40), (96, 0, 3, 77), (128, 0, 2, 40), (320, 0, 1, 81), (320, 640, 2, 35)])
def test_groupnorm_scale_shift_is_what_apply_uses(ops, c1, c2, n, hw):
    """gn_finalize_kernel: scale / shift inside their bound, and BITWISE the pair gn_apply_kernel multiplies by — half(x * sc + sh) in fp32
    reproduces the device's y exactly (silu = 0)."""
    for eps in (1e-5, 1e-6):
        x1, x2, ga, be = gn_input(n, hw, c1, c2, 31)
        sc, sh = ops.group_norm_scale_shift(x1, ga, be, eps, x2)
        sc_ref, sc_b, sh_ref, sh_b = EB.groupnorm_scale_shift_ref(x1, x2, ga, be, eps)
        held(sc, sc_ref, sc_b, f"gn scale C={c1}+{c2} hw={hw} eps={eps}")
        held(sh, sh_ref, sh_b, f"gn shift C={c1}+{c2} hw={hw} eps={eps}")
        y = ops.group_norm(x1, ga, be, eps, False, x2)
        x = x1 if x2 is None else torch.cat([x1, x2], dim=-1)
        fused, unfused = _fma_or_mul_add(x.reshape(n, hw, -1), sc.unsqueeze(1), sh.unsqueeze(1))
        y = y.reshape(n, hw, -1)
        assert torch.equal(y, fused) or torch.equal(y, unfused), \
            f"{int((y != fused).sum())} / {int((y != unfused).sum())} of {y.numel()} elements differ from half(x * sc + sh) (fused / unfused)"


def _rechunk(part, pstat, seed):
    """A producer's view of the same statistics: the per-image totals of `part` [n][P][32][2] split over pstat chunks in fp64, rounded to fp32."""
    total = part.double().sum(dim=1, keepdim=True)                               # [n][1][32][2]
    g = torch.Generator().manual_seed(seed)
    w = (torch.rand(pstat, generator=g, dtype=torch.float64) + 0.1).to(part.device)
    w = (w / w.sum()).reshape(1, pstat, 1, 1)
    out = (total * w).float()
    out[:, -1] = (total[:, 0] - out[:, :-1].double().sum(dim=1)).float()         # the last chunk takes what rounding left over
    return out.contiguous()


@pytest.mark.parametrize("c,lpg", [(64, 8), (128, 16), (320, 32)])
def test_groupnorm_from_partials(ops, c, lpg):
    """stats_ready > 0 with a producer's chunk count Pstat != P: the final reductions sweep Pstat in batches of 4 * lpg (lpg = 8 / 16 / 32 lanes per group
    for 1 / 2 / 4 channel slabs).  With the device's own partials and Pstat == P the result is bitwise the two-launch one."""
    n, hw, eps = 2, 77, 1e-5
    x1, _, ga, be = gn_input(n, hw, c, 0, 41)
    part = ops.group_norm_stats(x1)
    for silu in (False, True):
        y2 = ops.group_norm(x1, ga, be, eps, silu)
        assert torch.equal(ops.group_norm_from_partials(x1, part, ga, be, eps, silu), y2)
    sc0, sh0 = ops.group_norm_scale_shift(x1, ga, be, eps)
    sc1, sh1 = ops.group_norm_scale_shift(x1, ga, be, eps, part=part)
    assert torch.equal(sc0, sc1) and torch.equal(sh0, sh1)
    ref, bound = EB.groupnorm_ref(x1, None, ga, be, eps, True)
    sc_ref, sc_b, sh_ref, sh_b = EB.groupnorm_scale_shift_ref(x1, None, ga, be, eps)
    for pstat in (1, lpg - 1, lpg, 4 * lpg + 1, 1024):
        pp = _rechunk(part, pstat, pstat)
        y = ops.group_norm_from_partials(x1, pp, ga, be, eps, True)
        held(y.reshape(ref.shape), ref, bound, f"groupnorm from partials C={c} Pstat={pstat}")
        sc, sh = ops.group_norm_scale_shift(x1, ga, be, eps, part=pp)
        held(sc, sc_ref, sc_b, f"gn scale from partials C={c} Pstat={pstat}")
        held(sh, sh_ref, sh_b, f"gn shift from partials C={c} Pstat={pstat}")


# ------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("c", [8, 64, 320, 520, 2048])       # C = 520: CH = 65 chunks, lane 0 alone holds a second one; 2048: the largest accepted
@pytest.mark.parametrize("rows", [1, 5, 130])                # 130: 33 blocks of 4 waves, the last half empty
def test_layernorm(ops, c, rows):
    g = torch.Generator().manual_seed(c + rows)
    x = torch.randn(rows, c, generator=g)
    kind = torch.arange(rows) % 3
    x[kind == 1] += 100.0                                    # mu / sigma = 100
    x[kind == 2] = torch.randn(int((kind == 2).sum()), 1, generator=g) * 3.0        # constant rows
    x = x.half().to(DEV)
    ga = (1.0 + 0.5 * torch.randn(c, generator=g)).half().to(DEV)
    be = (0.5 * torch.randn(c, generator=g)).half().to(DEV)
    y = ops.layer_norm(x, ga, be, 1e-5)
    ref, bound = EB.layernorm_ref(x, ga, be, 1e-5)
    held(y, ref, bound, f"layernorm rows={rows} C={c}")


def test_layernorm_rejects_more_than_2048_channels(ops):
    x = torch.zeros(4, 2056, dtype=torch.float16, device=DEV)
    with pytest.raises(LDError) as e:
        ops.layer_norm(x, x[0].clone(), x[0].clone(), 1e-5)
    assert e.value.status == ERR_SHAPE


# ------------------------------------------------------------------ softmax
SENTINEL = 0x7BCD        # bits of the elements between cols and ld (a finite fp16 no softmax writes)


@pytest.mark.parametrize("cols", [8, 40, 2048, 2056, 4096])  # 2048: every thread exactly one chunk; 2056: thread 0 a second one
@pytest.mark.parametrize("rows", [1, 300])
def test_softmax_rows(ops, cols, rows):
    g = torch.Generator().manual_seed(cols + rows)
    for kind in ("scale4", "near+-60000"):
        base = torch.randn(rows, cols, generator=g) * 4.0
        if kind != "scale4":
            sign = torch.where(torch.arange(rows) % 2 == 0, 1.0, -1.0).reshape(rows, 1)
            base = sign * 60000.0 + torch.randn(rows, cols, generator=g) * 40.0
        for valid in (cols, cols - 1, cols - 7, 1):
            for ld in (cols, cols + 8):
                s = torch.full((rows, ld), 0.0).half()
                s[:, :cols] = base.half()
                if valid < cols:                 # the row's maximum sits in the pad columns: it must be ignored
                    s[:, valid:cols] = (s[:, :valid].float().amax(-1, keepdim=True) + 64.0).half() if kind == "scale4" else 65504.0
                s = s.to(DEV)
                s.view(torch.int16)[:, cols:] = SENTINEL
                ref, bound = EB.softmax_ref(s[:, :cols], valid)
                y = (ops.softmax_rows_ld_(s.clone(), cols, valid) if (ld != cols or valid != cols) else ops.softmax_rows_(s.clone()))
                what = f"softmax {kind} rows={rows} cols={cols} valid={valid} ld={ld}"
                assert bool((y.view(torch.int16)[:, cols:] == SENTINEL).all()), what + ": elements between cols and ld were written"
                assert bool((y[:, valid:cols] == 0).all()), what + ": pad columns must be exactly 0"
                keep = EB.top_half_per_row(ref)            # the bias statistic over the largest 50 % of every row's probabilities
                held(y[:, :cols], ref, bound, what, keep=keep, bias_extra=EB.subnormal_bias_allowance(ref, keep))
