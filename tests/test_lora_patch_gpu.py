"""GPU: LoRA patches of the RESIDENT weights — the merge kernel element-wise against fp64, the three resident layouts through patch /
read-back / unpatch, the reference's own patched weights, and the node path (`LoraLoader` on a loaded stack: clone and base share one
resident UNet / text model, swapped lazily), eager and through the captured hipGraph.

The element bound of the merge (dst = round_fp16(float(base) + sum_j s_j up_j down_j), fp32 products and sum, one rounding), against fp64 from
the same inputs, y_hat = base + sum s up down and A = |base| + sum |s| |up| |down|:
    e32   = (sum of ranks + 2) * 2^-24 * A        worst case of ANY fp32 summation order of the products onto the base
    bound = 2^-11 * (|y_hat| + e32) + e32 + 2^-24   one fp16 rounding (to nearest) of the fp32 result
and errbound.check holds the signed bias to BIAS_TOL as well (a truncating conversion fails it)."""
import ctypes as C

import numpy as np
import pytest
import torch

import errbound as E
from conftest import load_golden, rel_l2
from lightdiffusion_amd import weights as W

pytestmark = pytest.mark.gpu
# the kernels of lora.hip and the tests that hold them, element-wise and bitwise (tests/test_errbound_cpu.py keeps the ledger)
KERNELS = {"lora_merge_kernel": ["test_lora_merge_elementwise_against_fp64"], "lora_read_kernel": ["test_layout_round_trip_patch_read_unpatch"]}
DEV = "cuda:0"
UNET_TOL = 5e-3          # tests/test_configs_gpu.py: test_lora_merged_unet_and_clip_match_reference
CLIP_TOL = 5e-3
P = "model.diffusion_model."
TO_Q = "input_blocks.1.1.transformer_blocks.0.attn1.to_q.weight"
CONV1 = "input_blocks.1.0.in_layers.2.weight"
GEGLU = "input_blocks.1.1.transformer_blocks.0.ff.net.0.proj.weight"
TO_Q_LORA = "lora_unet_input_blocks_1_1_transformer_blocks_0_attn1_to_q"


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _terms(terms):
    """[(up, down, scale)] device tensors (fp16 or fp32, 2-D) -> ctypes array of ld_lora_term"""
    from lightdiffusion_amd._lib import F16, F32, LoraTerm
    arr = (LoraTerm * max(1, len(terms)))()
    for j, (up, down, s) in enumerate(terms):
        assert up.is_contiguous() and down.is_contiguous() and up.dtype == down.dtype
        arr[j].up, arr[j].down = up.data_ptr(), down.data_ptr()
        arr[j].dtype, arr[j].rank, arr[j].scale = (F32 if up.dtype == torch.float32 else F16), up.shape[1], s
    return arr


def _ref_and_bound(base, terms):
    """fp64 y_hat and the element bound of the module docstring; base [rows][cols], terms [(up [rows][r], down [r][cols], scale)]"""
    y = base.double()
    a = base.double().abs()
    ranks = 0
    for up, down, s in terms:
        s = float(np.float32(s))                                    # the scale crosses the ABI as a float
        y = y + s * (up.double() @ down.double())
        a = a + abs(s) * (up.double().abs() @ down.double().abs())
        ranks += up.shape[1]
    e32 = (ranks + 2) * 2.0 ** -24 * a
    return y, 2.0 ** -11 * (y.abs() + e32) + e32 + 2.0 ** -24


def _random_terms(gen, rows, cols, ranks, dtypes, scale=0.7):
    out = []
    for r, dt in zip(ranks, dtypes):
        up = (torch.randn(rows, r, generator=gen) * r ** -0.25).to(dt).to(DEV)
        down = (torch.randn(r, cols, generator=gen) * r ** -0.25).to(dt).to(DEV)
        out.append((up, down, scale))
    return out


@pytest.mark.parametrize("rows,cols,ranks,dtypes,inplace", [
    (96, 200, (4,), (torch.float32,), False),
    (160, 320, (16, 16), (torch.float16, torch.float32), True),       # one fp16 and one fp32 term; in place
    (33, 72, (1,), (torch.float32,), False),                          # ragged, cols not a multiple of 8
    (64, 64, (128,), (torch.float16,), False),
    (64, 576, (8,), (torch.float32,), True),
    (5, 36, (3,), (torch.float32,), False),
])
def test_lora_merge_elementwise_against_fp64(rows, cols, ranks, dtypes, inplace):
    from lightdiffusion_amd._lib import check, lib
    gen = torch.Generator().manual_seed(rows * 1000 + cols)
    base = torch.randn(rows, cols, generator=gen).half().to(DEV)
    terms = _random_terms(gen, rows, cols, ranks, dtypes)
    y_hat, bound = _ref_and_bound(base, terms)
    dst = base.clone() if inplace else torch.full_like(base, float("nan"))
    src = dst if inplace else base
    check(lib().ld_op_lora_merge(src.data_ptr(), dst.data_ptr(), rows, cols, _terms(terms), len(terms), _stream()), "ld_op_lora_merge")
    r, s = E.check(dst, y_hat, bound, f"lora merge {rows}x{cols} ranks {ranks}")
    print(f"lora merge {rows}x{cols} ranks {ranks}: worst error / bound {r:.3f}, signed bias {s:.2e}")
    if not inplace:
        assert torch.equal(src, base)


@pytest.fixture(scope="module")
def stack():
    """the set-up of test_lora_merged_unet_and_clip_match_reference, loaded WITHOUT the LoRA: tiny synthetic checkpoint, fp32 UNet base"""
    from lightdiffusion_amd import nodes
    from test_host_cpu import _lora_from_golden, _synthetic_checkpoint
    g = load_golden("lora_tiny")
    sd, ucfg, vcfg, ccfg = _synthetic_checkpoint()
    sd.update({P + k: v for k, v in W.synth_state_dict(W.unet_param_shapes(ucfg)).items()})
    loader = nodes.CheckpointLoaderSimple(DEV, max_batch=1, max_hw=(16, 16), clip_heads=ccfg["num_attention_heads"])
    model, clip, _ = loader.load_checkpoint(dict(sd))
    yield model, clip, sd, g, _lora_from_golden(g)
    del model, clip
    torch.cuda.empty_cache()


def _unet(model):
    return model.model.diffusion_model


@pytest.mark.parametrize("name", [TO_Q, CONV1, GEGLU])
def test_layout_round_trip_patch_read_unpatch(stack, name):
    from lightdiffusion_amd._lib import check, lib
    model, _, sd, _, _ = stack
    model.patch_model()
    u = _unet(model)
    first = u.read_param(name)
    assert torch.equal(first.cpu(), sd[P + name].half())                       # the load-time repack, undone bit for bit
    assert u.patch_bytes == 0
    rows, cols = first.shape[0], first[0].numel()
    gen = torch.Generator().manual_seed(len(name))
    terms = _random_terms(gen, rows, cols, (4,), (torch.float32,), scale=0.5)
    y_hat, bound = _ref_and_bound(first.reshape(rows, cols), terms)
    check(lib().ld_unet_patch_param(u._h, name.encode(), _terms(terms), 1, _stream()), "ld_unet_patch_param")
    assert u.patch_bytes == 2 * first.numel()
    E.check(u.read_param(name).reshape(rows, cols), y_hat, bound, f"patched {name} in checkpoint layout")
    # patching again recomputes from the backup: same terms, same bits (not cumulative)
    once = u.read_param(name)
    check(lib().ld_unet_patch_param(u._h, name.encode(), _terms(terms), 1, _stream()), "ld_unet_patch_param")
    assert torch.equal(u.read_param(name), once) and u.patch_bytes == 2 * first.numel()
    check(lib().ld_unet_unpatch(u._h, name.encode(), _stream()), "ld_unet_unpatch")
    assert torch.equal(u.read_param(name), first) and u.patch_bytes == 0
    check(lib().ld_unet_unpatch(u._h, name.encode(), _stream()), "ld_unet_unpatch")      # never patched: a no-op
    check(lib().ld_unet_refresh_derived(u._h, _stream()), "ld_unet_refresh_derived")   # (the raw C calls bypass the host mirror, which does this)


def test_patched_weights_match_the_reference_patcher(stack):
    """the golden's LoRA at strength 0.8 through LoraLoader: read-back against the weights the reference's ModelPatcher produced (fp32), one
    rounding of the fp32 base and one of the result allowed; the 3x3 pair pins the conv flatten order against the reference itself"""
    from lightdiffusion_amd import nodes
    model, clip, sd, g, lora = stack
    with pytest.warns(UserWarning, match="match no layer"):
        m1, _ = nodes.LoraLoader().load_lora(model, clip, lora, 0.8, 0.6)
    m1.patch_model()
    u = _unet(model)
    for name, ref in ((TO_Q, g["w_attn1_to_q"]), (CONV1, g["w_conv1"])):
        got, base = u.read_param(name).cpu().double(), sd[P + name].double()
        assert float((ref.double() - base).abs().max()) > 1e-3                     # (the fixture patches this weight)
        tol = 2.0 ** -11 * (base.abs() + ref.double().abs()) + 2.0 ** -24
        worst = float(((got - ref.double()).abs() / tol).max())
        print(f"{name}: worst error / tolerance {worst:.3f}")
        assert worst <= 1.0, (name, worst)
    model.patch_model()
    assert u.patch_bytes == 0 and u.applied_patches_uuid is None


def test_lora_through_the_node_after_a_plain_load(stack):
    from lightdiffusion_amd import nodes
    model, clip, sd, g, lora = stack
    u = _unet(model)
    x, sigma, ctx = g["x"].to(DEV), g["sigma"].to(DEV), g["ctx"]
    run = lambda m: m.model.apply_model(x, sigma, c_crossattn=ctx).cpu()          # ONE context object for every call below
    toks = [[(int(t), 1.0) for t in g["tokens"][0]]]
    inter = lambda c: c.patch_model()(g["tokens"], intermediate_output=-2)[1].cpu()
    den0, cond0, inter0 = run(model), clip.encode_from_tokens(toks), inter(clip)
    assert rel_l2(den0, g["denoised"]) > 2e-2                                      # the fixture is not a no-op
    with pytest.warns(UserWarning, match="match no layer"):
        m1, c1 = nodes.LoraLoader().load_lora(model, clip, lora, 0.8, 0.6)
    assert _unet(m1) is u and c1.text_model is clip.text_model and u.patch_bytes == 0      # nothing merged yet: the swap is lazy
    epoch = u.reserve_epoch
    den1 = run(m1)
    e_unet = rel_l2(den1, g["denoised"])
    inter1 = inter(c1)
    e_clip = rel_l2(inter1, g["clip_inter_m2"])
    print(f"device patch: UNet rel-L2 {e_unet:.3e}, CLIP rel-L2 {e_clip:.3e}")
    assert e_unet < UNET_TOL                                                       # (stale K / V^T would fail this: the fixture patches attn2.to_k)
    assert e_clip < CLIP_TOL
    assert u.patch_bytes > 0 and u.applied_patches_uuid == m1.patches_uuid
    cond1 = c1.encode_from_tokens(toks)
    # the base model again: the loaded weights bit for bit, UNet and text model
    assert torch.equal(run(model), den0) and u.patch_bytes == 0
    assert torch.equal(clip.encode_from_tokens(toks), cond0) and torch.equal(inter(clip), inter0)
    # clone -> base -> clone: the patched state is reproducible bit for bit
    assert torch.equal(run(m1), den1) and torch.equal(c1.encode_from_tokens(toks), cond1) and torch.equal(inter(c1), inter1)
    assert not torch.equal(cond1, cond0)
    assert u.reserve_epoch == epoch
    model.patch_model()
    clip.patch_model()


def test_patch_under_a_captured_graph(stack):
    from lightdiffusion_amd import nodes
    model, clip, sd, g, lora = stack
    u = _unet(model)
    x, sigma, ctx = g["x"][:1].to(DEV), g["sigma"][:1].to(DEV), g["ctx"]
    token = ("test_lora_graph", 1)
    model.patch_model()
    rep0 = u.cfg_denoise(x, sigma, ctx, 6.5, token=token, use_graph=True)
    key = (1, 16, 16, 6.5, True)
    entry, graph, epoch = u._denoisers[key], u._denoisers[key]._graph, u.reserve_epoch
    assert graph is not None
    with pytest.warns(UserWarning, match="match no layer"):
        m1, _ = nodes.LoraLoader().load_lora(model, clip, lora, 0.8, 0.6)
    m1.patch_model()
    rep1 = u.cfg_denoise(x, sigma, ctx, 6.5, token=token, use_graph=True)
    assert u._denoisers[key] is entry and entry._graph is graph and u.reserve_epoch == epoch     # replayed, not re-captured
    eager1 = u.cfg_denoise(x, sigma, ctx, 6.5, token=token, use_graph=False)
    assert torch.equal(rep1, eager1) and not torch.equal(rep1, rep0)
    model.patch_model()
    assert torch.equal(u.cfg_denoise(x, sigma, ctx, 6.5, token=token, use_graph=True), rep0)
    assert u._denoisers[key] is entry and entry._graph is graph and u.reserve_epoch == epoch


def test_two_loras_stack_as_two_terms(stack):
    from lightdiffusion_amd import nodes
    model, clip, sd, g, _ = stack
    u = _unet(model)
    model.patch_model()
    gen = torch.Generator().manual_seed(7)
    mk = lambda alpha: {TO_Q_LORA + ".lora_up.weight": torch.randn(64, 4, generator=gen) * 0.7,
                        TO_Q_LORA + ".lora_down.weight": torch.randn(4, 64, generator=gen) * 0.7, TO_Q_LORA + ".alpha": torch.tensor(alpha)}
    la, lb = mk(2.0), mk(8.0)
    m1, c1 = nodes.LoraLoader().load_lora(model, clip, la, 0.8, 0.0)
    m2, _ = nodes.LoraLoader().load_lora(m1, c1, lb, -0.5, 0.0)
    assert [len(v) for v in m2.patches.values()] == [2] and c1.patches == {}
    m2.patch_model()
    stacked = u.read_param(TO_Q)
    terms = [(l[TO_Q_LORA + ".lora_up.weight"], l[TO_Q_LORA + ".lora_down.weight"], s * float(l[TO_Q_LORA + ".alpha"]) / 4)
             for l, s in ((la, 0.8), (lb, -0.5))]
    u.patch_weights({TO_Q: terms})
    assert torch.equal(u.read_param(TO_Q), stacked)
    y_hat, bound = _ref_and_bound(sd[P + TO_Q].half().to(DEV), [(a.to(DEV), b.to(DEV), s) for a, b, s in terms])
    E.check(stacked, y_hat, bound, "two stacked LoRAs on attn1.to_q")
    model.patch_model()
    assert torch.equal(u.read_param(TO_Q).cpu(), sd[P + TO_Q].half())


def test_refused_patches_leave_the_slot_unchanged(stack):
    from lightdiffusion_amd._lib import ERR_ARG, LoraTerm, lib
    model, _, sd, _, _ = stack
    model.patch_model()
    u = _unet(model)
    up, down = torch.randn(64, 256, device=DEV), torch.randn(256, 64, device=DEV)
    big_up, big_down = torch.randn(64, 257, device=DEV), torch.randn(257, 64, device=DEV)
    one = _terms([(up, down, 1.0)])
    bias = "input_blocks.1.1.transformer_blocks.0.attn1.to_out.0.bias"
    before, bias_before = u.read_param(TO_Q), u.read_param(bias)
    rank0 = _terms([(up, down, 1.0)])
    rank0[0].rank = 0
    nine = _terms([(up[:, :4].contiguous(), down[:4].contiguous(), 0.1)] * 9)
    cases = [("unknown name", b"no.such.weight", one, 1), ("rank 0", TO_Q.encode(), rank0, 1),
             ("rank 257", TO_Q.encode(), _terms([(big_up, big_down, 1.0)]), 1), ("9 terms", TO_Q.encode(), nine, 9),
             ("0 terms", TO_Q.encode(), one, 0), ("bias slot", bias.encode(), one, 1)]
    for what, name, arr, n in cases:
        assert lib().ld_unet_patch_param(u._h, name, arr, n, _stream()) == ERR_ARG, what
        assert torch.equal(u.read_param(TO_Q), before) and torch.equal(u.read_param(bias), bias_before) and u.patch_bytes == 0, what
    assert lib().ld_op_lora_merge(before.data_ptr(), before.data_ptr(), 64, 64, nine, 9, _stream()) == ERR_ARG
    assert lib().ld_unet_unpatch(u._h, b"no.such.weight", _stream()) == ERR_ARG
    assert torch.equal(bias_before.cpu(), sd[P + bias].half())


def test_ksampler_swaps_the_clone_in_and_the_base_back(stack):
    """the product path: KSampler2 -> common_ksampler -> CFGGuider.sample takes the inner model through patch_model, so sampling with the
    LoRA clone and with the base alternately on ONE resident UNet gives each its own weights, reproducibly bit for bit"""
    from lightdiffusion_amd import nodes
    model, clip, sd, g, lora = stack
    u = _unet(model)
    ctx = g["ctx"]
    pos, neg = [[ctx[1:2], {"pooled_output": None}]], [[ctx[:1], {"pooled_output": None}]]
    lat = nodes.EmptyLatentImage().generate(128, 128, 1)[0]
    sample = lambda m: nodes.KSampler2().sample(m, 11, 2, 6.5, "euler_ancestral", "normal", pos, neg, lat)[0]["samples"]
    base = sample(model)
    assert u.patch_bytes == 0 and u.applied_patches_uuid is None and bool(torch.isfinite(base).all())
    with pytest.warns(UserWarning, match="match no layer"):
        m1, _ = nodes.LoraLoader().load_lora(model, clip, lora, 0.8, 0.0)
    assert u.patch_bytes == 0                                                      # lazy: nothing merged before the clone samples
    out1 = sample(m1)
    assert u.patch_bytes > 0 and u.applied_patches_uuid == m1.patches_uuid
    assert bool(torch.isfinite(out1).all()) and not torch.equal(out1, base)
    assert torch.equal(sample(model), base) and u.patch_bytes == 0 and u.applied_patches_uuid is None
    assert torch.equal(sample(m1), out1)
    model.patch_model()


def test_load_param_onto_a_patched_slot_is_the_new_base(stack):
    from lightdiffusion_amd._lib import F16, check, lib
    model, _, sd, _, _ = stack
    model.patch_model()
    u = _unet(model)
    first = u.read_param(TO_Q)
    gen = torch.Generator().manual_seed(3)
    u.patch_weights({TO_Q: [(torch.randn(64, 4, generator=gen), torch.randn(4, 64, generator=gen), 0.5)]})
    assert u.patch_bytes == 2 * first.numel() and not torch.equal(u.read_param(TO_Q), first)
    new = (first.float() * 0.5).half().contiguous()
    check(lib().ld_unet_load_param(u._h, TO_Q.encode(), new.data_ptr(), F16, _stream()), "ld_unet_load_param")
    assert u.patch_bytes == 0 and torch.equal(u.read_param(TO_Q), new)           # the backup is dropped with the load
    model.patch_model()                                                            # the lazy restore finds nothing to copy back
    assert u.patch_bytes == 0 and u.applied_patches_uuid is None and torch.equal(u.read_param(TO_Q), new)
    check(lib().ld_unet_load_param(u._h, TO_Q.encode(), first.data_ptr(), F16, _stream()), "ld_unet_load_param")   # (the shared stack as it was)
    check(lib().ld_unet_refresh_derived(u._h, _stream()), "ld_unet_refresh_derived")
    assert torch.equal(u.read_param(TO_Q).cpu(), sd[P + TO_Q].half())


def test_a_refused_patch_set_rolls_back_unet_and_text_model(stack):
    """a failure part-way through a patch set (factors of the wrong shape: refused on the host before the kernel could index them out of
    bounds; a rank the library refuses) leaves the LOADED weights, on the UNet and on the text model with its fused q|k|v copy"""
    from lightdiffusion_amd._lib import LDError
    model, clip, sd, _, _ = stack
    model.patch_model()
    clip.patch_model()
    u, tm = _unet(model), clip.text_model
    gen = torch.Generator().manual_seed(5)
    rnd = lambda *s: torch.randn(*s, generator=gen) * 0.3
    q0, c0 = u.read_param(TO_Q), u.read_param(CONV1)
    good = [(rnd(64, 4), rnd(4, 64), 0.5)]
    for bad, err in (([(rnd(64, 4), rnd(4, 32, 3, 3), 0.5)], ValueError),          # smaller than the slot: would be read out of bounds
                     ([(rnd(64, 4), rnd(4, 96, 3, 3), 0.5)], ValueError),          # larger: would merge wrong weights silently
                     ([(rnd(32, 4), rnd(4, 64, 3, 3), 0.5)], ValueError),
                     ([(rnd(64, 257), rnd(257, 64, 3, 3), 0.5)], LDError)):
        with pytest.raises(err):
            u.patch_weights({TO_Q: good, CONV1: bad}, uuid="never applied")
        assert u.patch_bytes == 0 and u.applied_patches_uuid is None
        assert torch.equal(u.read_param(TO_Q), q0) and torch.equal(u.read_param(CONV1), c0)
    with pytest.raises(KeyError):
        u.patch_weights({TO_Q: good, "no.such.weight": good})
    assert u.patch_bytes == 0 and torch.equal(u.read_param(TO_Q), q0)
    # the text model
    kq, kk = ("text_model.encoder.layers.0.self_attn.%s_proj.weight" % t for t in "qk")
    h = tm.w[kq].shape[0]
    wq, wk, fused = tm.w[kq].clone(), tm.w[kk].clone(), tm.qkv[0][0].clone()
    tgood = [(rnd(h, 4), rnd(4, h), 0.5)]
    for bad, err in (([(rnd(h, 4), rnd(4, h // 2), 0.5)], ValueError), ([(rnd(h, 257), rnd(257, h), 0.5)], LDError)):
        with pytest.raises(err):
            tm.patch_weights({kq: tgood, kk: bad}, uuid="never applied")
        assert tm.applied_patches_uuid is None and tm._backup == {}
        assert torch.equal(tm.w[kq], wq) and torch.equal(tm.w[kk], wk) and torch.equal(tm.qkv[0][0], fused)
    tm.patch_weights({kq: tgood})                                                  # (the same terms do patch when the set is sound)
    assert not torch.equal(tm.w[kq], wq) and not torch.equal(tm.qkv[0][0], fused)
    clip.patch_model()
    assert torch.equal(tm.w[kq], wq) and torch.equal(tm.qkv[0][0], fused)
