"""GPU: the boundary convolutions, the timestep embedding, the CFG-pair plumbing, the samplers' elementwise arithmetic and the weight folds of misc.hip, each held element-wise
(tests/errbound.py) against an fp64 reference from the same inputs, or bitwise where the kernel only moves or compares data.  The two small
convolutions pin the instantiation they ran through ld_op_last_kernel.  Each case prints its worst error / bound and signed bias.

KERNELS names, per kernel, the tests that hold it (tests/test_errbound_cpu.py checks that no kernel of misc.hip is missing)."""
import math

import pytest
import torch

import errbound as EB
from conftest import load_golden
from lightdiffusion_amd._lib import ERR_ARG, ERR_SHAPE, F16, F32, OK, LDError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

KERNELS = {
    "small_conv_in_kernel": ["test_small_conv_in", "test_small_conv_in_second_lap", "test_small_conv_in_dup_off"],
    "small_conv_out_kernel": ["test_small_conv_out", "test_small_conv_out_many_laps", "test_small_conv_out_in_mod"],
    "small_pointwise_kernel": ["test_small_pointwise"],
    "vae_out_finish_kernel": ["test_vae_out_finish"],
    "timestep_embed_kernel": ["test_timestep_embed"],
    "dup_halves_kernel": ["test_dup_halves"],
    "ctx_pad_kernel": ["test_ctx_pad"],
    "hook_check_kernel": ["test_hook_check"],
    "ln_fold_kernel": ["test_ln_fold"],
    "mlp_out_fold_kernel": ["test_mlp_out_fold"],
    "repack_conv3x3_kernel": ["test_repack_conv_is_a_permutation"],
    "cfg_combine_kernel": ["test_cfg_combine"],
    "axpby_kernel": ["test_axpby"],
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


def rnd(shape, g, scale=1.0, dtype=torch.float16):
    return (torch.randn(shape, generator=g) * scale).to(dtype).to(DEV)


def status(fn):
    try:
        fn()
    except LDError as e:
        return e.status
    return OK


# ------------------------------------------------------------------ small_conv_out
# Cin -> the instantiation: ceil(9 (Cin / 8) / 64) chunks per lane, <3,4> up to 3, <6,2> up to 6, <9,1> beyond.  Ownership edges inside a variant: Cin = 8 — nine
# lanes own one chunk each; 128 — 144 chunks, lanes 0..15 own three and the rest two; 192 — 216, lanes 0..23 own four; 384 — 432, lanes 0..47 own seven; 512 — all nine
OUT_VARIANT = {8: "small_conv_out_kernel<3,4>", 64: "small_conv_out_kernel<3,4>", 128: "small_conv_out_kernel<3,4>", 192: "small_conv_out_kernel<6,2>",
               320: "small_conv_out_kernel<6,2>", 384: "small_conv_out_kernel<9,1>", 512: "small_conv_out_kernel<9,1>"}
SIGMAS = (0.03, 14.6)


def conv_out_case(ops, x, cout, mode, g, what):
    n, h, w, cin = x.shape
    wt = rnd((cout, 9 * cin), g, 1.0 / math.sqrt(9 * cin))
    b = (torch.tensor([1.5, -1.25, 2.0, -1.75])[:cout] if mode != 1 else torch.tensor([0.5, -0.375, 0.25, -0.5])[:cout]).half().to(DEV)
    x_in = sigma = None
    if mode == 0:
        x_in = rnd((n, cout, h, w), g, 1.0, torch.float32)
        sigma = torch.tensor([SIGMAS[i % 2] for i in range(n)], dtype=torch.float32, device=DEV)
    y = ops.small_conv_out(x, wt, b, mode, x_in, sigma)
    assert ops.last_kernel() == OUT_VARIANT[cin], (ops.last_kernel(), cin)
    ref, bound = EB.small_conv_out_ref(x, wt, b, mode, x_in, sigma)
    held(y.reshape(ref.shape), ref, bound, f"{OUT_VARIANT[cin]} {what} Cout={cout} mode={mode}")
    if mode == 1:
        return float((ref == 0).double().mean() + (ref == 1).double().mean())
    return 0.0


# 1 x 5 x 7: 35 pixels, ragged against PX = 4 and 2; one row; one column; two images of 16 x 16 (the image index in the pixel decomposition)
@pytest.mark.parametrize("n,h,w", [(1, 5, 7), (1, 1, 9), (1, 9, 1), (2, 16, 16)])
@pytest.mark.parametrize("cin", sorted(OUT_VARIANT))
def test_small_conv_out(ops, cin, n, h, w):
    g = torch.Generator().manual_seed(cin * 1000 + h * 10 + w)
    x = rnd((n, h, w, cin), g)
    clamped = 0.0
    for cout in (1, 3, 4):
        for mode in (0, 1, 2):
            clamped = max(clamped, conv_out_case(ops, x, cout, mode, g, f"{n}x{h}x{w} Cin={cin}"))
    assert clamped > 0.0 or n * h * w < 30, "mode 1: no output reached the clamp"
    print(f"pinned {OUT_VARIANT[cin]}")


@pytest.mark.parametrize("cin", [8, 384])
def test_small_conv_out_many_laps(ops, cin):
    """1 x 200 x 200: 40000 pixels, several laps of every wave's grid-stride loop."""
    g = torch.Generator().manual_seed(cin)
    x = rnd((1, 200, 200, cin), g)
    for cout, mode in ((4, 0), (3, 1), (4, 2)):
        conv_out_case(ops, x, cout, mode, g, f"1x200x200 Cin={cin}")
    print(f"pinned {OUT_VARIANT[cin]}")


@pytest.mark.parametrize("cin", [64, 320, 512])
def test_small_conv_out_in_mod(ops, cin):
    """mode 0 with in_mod = 2 at N = 4 (a CFG pair: samples 2, 3 read x_in / sigma of 0, 1): the reference, and bitwise the call on explicitly
    duplicated x_in and sigma."""
    g = torch.Generator().manual_seed(cin + 1)
    x = rnd((4, 5, 7, cin), g)
    wt, b = rnd((4, 9 * cin), g, 1.0 / math.sqrt(9 * cin)), torch.tensor([1.5, -1.25, 2.0, -1.75]).half().to(DEV)
    x_in = rnd((2, 4, 5, 7), g, 1.0, torch.float32)
    sigma = torch.tensor(SIGMAS, dtype=torch.float32, device=DEV)
    y = ops.small_conv_out(x, wt, b, 0, x_in, sigma, in_mod=2)
    assert ops.last_kernel() == OUT_VARIANT[cin]
    ref, bound = EB.small_conv_out_ref(x, wt, b, 0, x_in, sigma, in_mod=2)
    held(y, ref, bound, f"{OUT_VARIANT[cin]} in_mod=2 N=4")
    assert torch.equal(y, ops.small_conv_out(x, wt, b, 0, x_in.repeat(2, 1, 1, 1), sigma.repeat(2)))


def test_small_conv_out_rejects(ops):
    g = torch.Generator().manual_seed(5)
    mk = lambda cin, cout: ops.small_conv_out(rnd((1, 4, 4, cin), g), rnd((cout, 9 * cin), g), rnd((cout,), g), 2)
    assert status(lambda: mk(520, 4)) == ERR_SHAPE and ops.last_kernel() == ""
    assert status(lambda: mk(64, 5)) == ERR_SHAPE and ops.last_kernel() == ""
    assert status(lambda: ops.small_conv_out(rnd((1, 4, 4, 64), g), rnd((4, 576), g), rnd((4,), g), 0)) == ERR_ARG     # mode 0 without x_in / sigma


# ------------------------------------------------------------------ small_conv_in
def conv_in_case(ops, n, cin, h, w, cout, variant, g):
    x = rnd((n, cin, h, w), g, 1.0, torch.float32)
    wt, b = rnd((cout, 9 * cin), g, 1.0 / math.sqrt(9 * cin)), rnd((cout,), g, 1.0)
    sig = pw = pb = None
    if variant == "sigma":
        sig = torch.tensor([SIGMAS[i % 2] for i in range(n)], dtype=torch.float32, device=DEV)
    if variant == "pre":
        pw, pb = rnd((cin, cin), g, 0.7), rnd((cin,), g, 0.5)
    y = ops.small_conv_in(x, wt, b, sig, pw, pb)
    name = f"small_conv_in_kernel<{cin}>"
    assert ops.last_kernel() == name, ops.last_kernel()
    ref, bound = EB.small_conv_in_ref(x, wt, b, sig, pw, pb)
    held(y.reshape(ref.shape), ref, bound, f"{name} {variant} {n}x{h}x{w} Cout={cout}")
    return name


# <4> takes the 8-byte filter-bank prologue (36 is a multiple of 4); <1>, <2>, <3> (9, 18, 27 weights per row) the scalar one
@pytest.mark.parametrize("n,h,w", [(1, 1, 9), (1, 9, 1), (2, 5, 7)])
@pytest.mark.parametrize("cin", [1, 2, 3, 4])
def test_small_conv_in(ops, cin, n, h, w):
    g = torch.Generator().manual_seed(cin * 100 + h * 10 + w)
    for cout in (8, 64, 320):
        for variant in ("plain", "sigma") + (("pre",) if cin >= 3 else ()):
            name = conv_in_case(ops, n, cin, h, w, cout, variant, g)
    print(f"pinned {name}")


@pytest.mark.parametrize("cin,variant", [(4, "sigma"), (3, "pre")])
def test_small_conv_in_second_lap(ops, cin, variant):
    """2 x 64 x 64 at Cout = 320: 327680 (pixel, channel group) items against a grid of 1024 x 256 threads — the grid-stride loop's second lap."""
    conv_in_case(ops, 2, cin, 64, 64, 320, variant, torch.Generator().manual_seed(cin))


def test_small_conv_in_dup_off(ops):
    """dup_off: the second copy is bitwise the first, and the guard elements around both copies stay untouched."""
    g = torch.Generator().manual_seed(9)
    n, cin, h, w, cout, guard = 2, 4, 5, 7, 64, 64
    size = n * h * w * cout
    x = rnd((n, cin, h, w), g, 1.0, torch.float32)
    wt, b = rnd((cout, 36), g, 1.0 / 6), rnd((cout,), g)
    sig = torch.tensor(SIGMAS, dtype=torch.float32, device=DEV)
    buf = torch.full((3 * guard + 2 * size,), -7.5, dtype=torch.float16, device=DEV)
    ops.small_conv_in(x, wt, b, sig, y=buf[guard:guard + size], dup_off=size + guard)
    first, second = buf[guard:guard + size], buf[2 * guard + size:2 * guard + 2 * size]
    assert torch.equal(first, second)
    assert torch.equal(first, ops.small_conv_in(x, wt, b, sig).flatten())
    for a in (0, guard + size, 2 * guard + 2 * size):
        assert bool((buf[a:a + guard] == -7.5).all()), f"guard at {a} was written"


def test_small_conv_in_rejects(ops):
    g = torch.Generator().manual_seed(6)
    mk = lambda cin, cout: ops.small_conv_in(rnd((1, cin, 4, 4), g, 1.0, torch.float32), rnd((cout, 9 * cin), g), rnd((cout,), g))
    assert status(lambda: mk(5, 8)) == ERR_SHAPE and ops.last_kernel() == ""
    assert status(lambda: mk(4, 12)) == ERR_SHAPE and ops.last_kernel() == ""


# ------------------------------------------------------------------ small_pointwise, vae_out_finish
@pytest.mark.parametrize("n,hw", [(1, 1), (5, 7), (3, 100000)])
def test_small_pointwise(ops, n, hw):
    g = torch.Generator().manual_seed(hw)
    x, wt, b = rnd((n, hw, 8), g), rnd((8, 8), g, 0.4), rnd((8,), g, 0.5)
    y = ops.small_pointwise(x, wt, b)
    ref, bound = EB.small_pointwise_ref(x, wt, b)
    held(y, ref, bound, f"small_pointwise n={n} hw={hw}")
    assert status(lambda: ops.small_pointwise(x[..., :4].contiguous(), wt[:4, :4].contiguous(), b[:4].contiguous())) == ERR_SHAPE


@pytest.mark.parametrize("npix", [1, 35, 300000])
def test_vae_out_finish(ops, npix):
    g = torch.Generator().manual_seed(npix)
    t8 = rnd((npix, 8), g, 0.8)
    t8[0] = torch.tensor([-1.0, 1.0, -1.25, 1.25, -1.0009765625, 1.0009765625, 0.0, -0.99951171875]).half().to(DEV)
    for cout in (3, 8):
        y = ops.vae_out_finish(t8, cout)
        ref, bound = EB.vae_out_finish_ref(t8, cout)
        held(y, ref, bound, f"vae_out_finish npix={npix} cout={cout}", keep=torch.ones_like(ref, dtype=torch.bool))
        assert y[0, :3].tolist() == [0.0, 1.0, 0.0]                     # the clamp at exactly -1, +1 and beyond
        if cout == 8:
            assert y[0, 3:6].tolist() == [1.0, 0.0, 1.0] and 0.0 < float(y[0, 7]) < 1e-3
        assert float(y.min()) >= 0.0 and float(y.max()) <= 1.0


# ------------------------------------------------------------------ timestep embedding
def _tables():
    tabs = {"sd15": load_golden("schedules")["log_sigmas"].float()}
    for n_sig in (1, 255, 257):
        tabs[f"n{n_sig}"] = torch.linspace(-3.5, 2.7, n_sig) if n_sig > 1 else torch.tensor([0.25])
    dup = torch.linspace(-3.5, 2.7, 257)
    dup[256] = dup[0]                    # both seen by thread 0 (i = 0 and i = 256)
    dup[200] = dup[3]                    # two threads, met in the tree reduction
    dup[4] = dup[3]                      # neighbours
    tabs["duplicates"] = dup
    return tabs


@pytest.mark.parametrize("dim", [2, 320, 1280])
def test_timestep_embed(ops, dim):
    for name, tab in _tables().items():
        n_sig = tab.numel()
        td = tab.double()
        picks = sorted({0, 1, n_sig // 3, n_sig - 2, n_sig - 1} & set(range(n_sig)))
        ls = [float(td[i]) for i in picks]                                                     # exactly from the table
        ls += [float(td[i] + 0.3 * (td[i + 1] - td[i])) for i in picks if i + 1 < n_sig and name != "duplicates"]   # between two entries, nearer the lower
        ls += [float(td.min()) - 3.0, float(td.max()) + 3.0]                                   # below and above the table
        if name == "duplicates":
            ls += [float(td[3]), float(td[0]), float(td[3]) + 1e-3]
        sigma = torch.tensor(ls, dtype=torch.float64).exp().float().to(DEV)
        t_ref, margin, emb_ref, bound = EB.timestep_ref(sigma, tab.to(DEV), dim)
        assert float(margin.min()) > 1e-4, f"{name}: an ill-posed case (margin {float(margin.min()):.2e}); change the inputs"
        emb, t = ops.timestep_embed(sigma, tab.to(DEV), dim)
        assert torch.equal(t.long(), t_ref), (name, t.long().tolist(), t_ref.tolist())
        if name == "duplicates":
            assert t_ref[-3:].tolist() == [3, 0, 3]                                            # ties go to the lowest index
        held(emb, emb_ref, bound, f"timestep_embed {name} dim={dim}", keep=torch.ones_like(emb_ref, dtype=torch.bool))
        # sigma_mod = 2 with N = 6: sample i reads sigma[i % 2]
        emb6, t6 = ops.timestep_embed_mod(sigma[:2].contiguous(), tab.to(DEV), dim, 6, 2)
        assert torch.equal(t6, t[:2].repeat(3)) and torch.equal(emb6, emb[:2].repeat(3, 1))


# ------------------------------------------------------------------ dup_halves, ctx_pad, hook_check, repack: bitwise
def test_dup_halves(ops):
    from lightdiffusion_amd._lib import lib
    g = torch.Generator().manual_seed(3)

    def rng(nbytes):
        t = torch.randint(0, 256, (2 * nbytes + 64,), generator=g, dtype=torch.uint8).to(DEV)
        return t, t.clone()

    def ok(t, before, nbytes):
        return torch.equal(t[nbytes:2 * nbytes], before[:nbytes]) and torch.equal(t[:nbytes], before[:nbytes]) and torch.equal(t[2 * nbytes:], before[2 * nbytes:])

    s = torch.cuda.current_stream().cuda_stream
    for nbytes in (16, 16 * 1023, 16 * 1025):               # one chunk; one short of a block's 1024; one chunk into the second block
        t, before = rng(nbytes)
        assert lib().ld_op_dup_halves(t.data_ptr(), nbytes, None, 0, None, 0, 1, s) == OK
        assert ok(t, before, nbytes), nbytes
    sizes = (16, 16 * 1025, 16 * 70000)                    # three ranges of very different length in one launch
    bufs = [rng(b) for b in sizes]
    assert lib().ld_op_dup_halves(bufs[0][0].data_ptr(), sizes[0], bufs[1][0].data_ptr(), sizes[1], bufs[2][0].data_ptr(), sizes[2], 3, s) == OK
    for (t, before), b in zip(bufs, sizes):
        assert ok(t, before, b), b
    t, before = rng(64)
    assert lib().ld_op_dup_halves(t.data_ptr() + 8, 16, None, 0, None, 0, 1, s) == ERR_ARG
    assert lib().ld_op_dup_halves(t.data_ptr(), 24, None, 0, None, 0, 1, s) == ERR_ARG
    assert lib().ld_op_dup_halves(t.data_ptr(), 16, None, 0, None, 0, 4, s) == ERR_ARG
    assert torch.equal(t, before)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_ctx_pad(ops, dtype):
    g = torch.Generator().manual_seed(8)
    for n, t, tp, d in ((2, 77, 80, 768), (3, 80, 80, 64), (1, 1, 8, 8)):
        src = rnd((n, t, d), g, 1.0, dtype)
        ref = torch.zeros(n, tp, d, dtype=torch.float16, device=DEV)
        ref[:, :t] = src.half()
        assert torch.equal(ops.ctx_pad(src, tp).view(torch.int16), ref.view(torch.int16)), (n, t, tp, d)
    assert status(lambda: ops.ctx_pad(src, 0)) == ERR_ARG


def test_hook_check(ops):
    """A correctness guard: a difference it misses means stale K / V.  One flipped bit in the first, a middle and the LAST word, in a buffer the
    grid-stride loop laps over (> 262144 words) and in one of three words; only the right flag changes and takes the passed epoch."""
    from lightdiffusion_amd._lib import lib
    g = torch.Generator().manual_seed(4)
    s = torch.cuda.current_stream().cuda_stream
    epoch = [100]

    def run(a, b, x, sig, half_sig):
        flags = torch.tensor([-7, -9], dtype=torch.int32, device=DEV)
        epoch[0] += 1
        st = lib().ld_op_hook_check(a.data_ptr(), b.data_ptr(), a.numel(), x.data_ptr(), x.numel() // 2, sig.data_ptr(), half_sig, flags.data_ptr(), epoch[0], s)
        assert st == OK
        return flags.tolist(), epoch[0]

    for words in (3, 300001):
        a = torch.randint(-2 ** 31, 2 ** 31 - 1, (words,), generator=g, dtype=torch.int64).to(torch.int32).to(DEV)
        xh = torch.randint(-2 ** 31, 2 ** 31 - 1, (words,), generator=g, dtype=torch.int64).to(torch.int32).to(DEV)
        x = torch.cat([xh, xh])
        sig = torch.tensor([0.5, 2.0, 7.0] * 2, dtype=torch.float32, device=DEV)
        f, e = run(a, a.clone(), x, sig, 3)
        assert f == [-7, -9], f
        for pos in (0, words // 2, words - 1):
            for bit in (0, 31):
                b = a.clone()
                b[pos] ^= (1 << bit) if bit < 31 else -2 ** 31
                f, e = run(a, b, x, sig, 3)
                assert f == [e, -9], (words, pos, bit, f)
                x2 = x.clone()
                x2[words + pos] ^= (1 << bit) if bit < 31 else -2 ** 31
                f, e = run(a, a.clone(), x2, sig, 3)
                assert f == [-7, e], (words, pos, bit, f)
        sig2 = sig.clone()
        sig2[5] = 7.000001                                            # only sigma[half_sig - 1] of the second half differs
        f, e = run(a, a.clone(), x, sig2, 3)
        assert f == [-7, e], f
    big = torch.arange(512, dtype=torch.float32, device=DEV)
    big2 = torch.cat([big[:256], big[:256]])
    assert run(a, a.clone(), x, big2, 256)[0] == [-7, -9]
    big2[511] = -1.0
    f, e = run(a, a.clone(), x, big2, 256)
    assert f == [-7, e]
    flags = torch.zeros(2, dtype=torch.int32, device=DEV)
    assert lib().ld_op_hook_check(a.data_ptr(), a.data_ptr(), 3, x.data_ptr(), 3, big2.data_ptr(), 257, flags.data_ptr(), 1, s) == ERR_SHAPE


def test_repack_conv_is_a_permutation(ops):
    from lightdiffusion_amd._lib import lib
    g = torch.Generator().manual_seed(2)
    for dtype, code in ((torch.float16, F16), (torch.float32, F32)):
        src = rnd((24, 40, 3, 3), g, 1.0, dtype)
        dst = torch.empty(24, 9, 40, dtype=torch.float16, device=DEV)
        assert lib().ld_op_repack_conv(src.data_ptr(), code, 24, 40, dst.data_ptr(), torch.cuda.current_stream().cuda_stream) == OK
        assert torch.equal(dst, src.half().reshape(24, 40, 9).permute(0, 2, 1).contiguous())


# ------------------------------------------------------------------ folds
@pytest.mark.parametrize("c", [64, 320])
def test_mlp_out_fold(ops, c):
    g = torch.Generator().manual_seed(c)
    wpo, w2 = rnd((c, c), g, 1.0 / math.sqrt(c)), rnd((c, 4 * c), g, 1.0 / math.sqrt(4 * c))
    b2, bpo = rnd((c,), g, 0.3), rnd((c,), g, 0.3)
    w_out, b_out = ops.mlp_out_fold(wpo, w2, b2, bpo)
    w_ref, w_b, b_ref, b_b = EB.mlp_out_fold_ref(wpo, w2, b2, bpo)
    held(w_out, w_ref, w_b, f"mlp_out_fold W' C={c}")
    held(b_out, b_ref, b_b, f"mlp_out_fold b' C={c}")
    assert torch.equal(w_out[:, 4 * c:].view(torch.int16), wpo.view(torch.int16))          # the identity columns are Wpo, bit for bit


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("n,k", [(192, 64), (960, 320), (7, 1280)])
def test_ln_fold(ops, n, k, bias):
    g = torch.Generator().manual_seed(n + k)
    w = rnd((n, k), g, 1.0 / math.sqrt(k))
    ga, be = (1.0 + 0.5 * torch.randn(k, generator=g)).half().to(DEV), rnd((k,), g, 0.5)
    b = rnd((n,), g, 0.3) if bias else None
    w_out, b_out, wsum = ops.ln_fold(w, ga, be, b)
    w_ref, w_b, b_ref, b_b = EB.ln_fold_ref(w, ga, be, b)
    held(w_out, w_ref, w_b, f"ln_fold W' N={n} K={k}")
    assert torch.equal(w_out, (w.float() * ga.float()).half())                             # an fp16 x fp16 product is exact in fp32: one rounding
    held(b_out, b_ref, b_b, f"ln_fold b' N={n} K={k} bias={bias}", keep=torch.ones_like(b_ref, dtype=torch.bool))
    s_ref, s_b = EB.wsum_ref(w_out)
    held(wsum, s_ref, s_b, f"ln_fold wsum N={n} K={k}", keep=torch.ones_like(s_ref, dtype=torch.bool))


# ------------------------------------------------------------------ the samplers' elementwise arithmetic
# grid_for caps these launches at 4096 blocks of 256 threads: 4096 * 256 + 3 elements are a full first lap and a second one of three elements
LAP = 4096 * 256
everything = lambda t: torch.ones_like(t, dtype=torch.bool)


@pytest.mark.parametrize("n_half", [5, LAP + 3])
def test_cfg_combine(ops, n_half):
    g = torch.Generator().manual_seed(n_half)
    den2 = rnd((2, n_half), g, 3.0, torch.float32)
    for cfg in (0.0, 1.0, 7.5, -2.0):
        out = ops.cfg_combine(den2, cfg)
        assert tuple(out.shape) == (1, n_half)
        ref, bound = EB.cfg_combine_ref(den2, cfg)
        held(out, ref, bound, f"cfg_combine n_half={n_half} cfg={cfg}", keep=everything(ref))
        if cfg == 0.0:
            assert torch.equal(out.view(torch.int32), den2[:1].view(torch.int32))       # u + (c - u) * 0 is u, bit for bit


@pytest.mark.parametrize("n", [5, LAP + 3])
def test_axpby(ops, n):
    """All four pointer arms (y / z present or null), fp32 scalars; a = 1, b = c = 0 leaves x as it is bit for bit in every arm."""
    g = torch.Generator().manual_seed(n + 1)
    x0, y, z = (rnd((n,), g, 2.0, torch.float32) for _ in range(3))
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))
    a, b, c = f32(0.7), f32(-1.3), f32(2.5)
    for yy, zz in ((y, z), (y, None), (None, z), (None, None)):
        x = x0.clone()
        assert ops.axpby_(x, a, yy, b, zz, c) is x
        ref, bound = EB.axpby_ref(x0, a, yy, b, zz, c)
        held(x, ref, bound, f"axpby n={n} y={yy is not None} z={zz is not None}", keep=everything(ref))
        x = x0.clone()
        ops.axpby_(x, 1.0, yy, 0.0, zz, 0.0)
        assert torch.equal(x.view(torch.int32), x0.view(torch.int32)), (n, yy is not None, zz is not None)
