"""GPU: ControlNet on the device against tests/controlnet_ref.py (upstream's cldm.ControlNet.forward and apply_control, fp32, on the blocks of
oracle/sd15_ref.py).  Tiny configuration, latents 16 x 16 (batch 1) and 8 x 24 (batch 2), the synthetic ControlNet, whose control moves the
reference's output by rel-L2 >= 0.05 (tests/test_controlnet_cpu.py holds that condition), so the 5e-3 comparisons tell control applied from
control ignored.
  executor   every residual on its own and the controlled UNet output below UNET_TOL = 5e-3, the project's per-call bound (the control branch is a
             strict prefix of a UNet call); strength 0 and all-zero zero convolutions are the plain forward's bits; the pair forms against the plain
             forms on duplicated inputs (1e-3, the existing bound of tests/test_models_gpu.py); a wrong count / shape / r_n is LD_ERR_SHAPE and
             writes nothing.
  sampler    apply_control=True over 4 euler_ancestral steps: graph replay is eager launches bit for bit; with the range (0.0, 0.5) every step is
             exactly the controlled step while sigma is inside the range and exactly the ordinary one after it; the hint is encoded once per run; a
             batch-1 hint serves batch 2; the handle's load -> unload -> load."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import controlnet_ref as R                                     # noqa: E402
from conftest import rel_l2                                    # noqa: E402
from lightdiffusion_amd import nodes as N                      # noqa: E402
from lightdiffusion_amd import sampling as S                   # noqa: E402
from lightdiffusion_amd import weights as W                    # noqa: E402
from lightdiffusion_amd._lib import ERR_ARG, ERR_SHAPE, LDError   # noqa: E402
from oracle import sd15_ref as O                               # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
UNET_TOL = 5e-3          # the per-call bound of tests/test_models_gpu.py
CFG = W.tiny_unet_config()
CASES = [(1, 16, 16), (2, 8, 24)]


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def case(b, h, w, seed=3, ctx_rows=None):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(b, 4, h, w, generator=g) * 3.0
    s = torch.tensor([2.5, 0.7][:b])
    ctx = torch.randn(ctx_rows or b, 77, CFG["context_dim"], generator=g)
    hint = torch.rand(1, 3, 8 * h, 8 * w, generator=g)
    return x, s, ctx, hint


@pytest.fixture(scope="module")
def unet():
    from lightdiffusion_amd.unet import synthetic_unet
    return synthetic_unet(CFG, max_batch=4, max_hw=(16, 24))


@pytest.fixture(scope="module")
def cnet():
    from lightdiffusion_amd.controlnet import synthetic_controlnet
    return synthetic_controlnet(CFG, max_batch=4, max_hw=(16, 24))


@pytest.fixture(scope="module")
def masters():
    return W.synth_state_dict(W.unet_param_shapes(CFG)), R.synth_state_dict(CFG), O.ModelSampling()


def branch(cnet, x, s, ctx, hint):
    """the control branch on the device -> its residuals as fp32 NCHW on the host"""
    cnet.set_context(ctx)
    cnet.set_hint(hint)
    cnet.forward(x.to(DEV), s.to(DEV))
    return [r.float().permute(0, 3, 1, 2).cpu() for r in cnet.residuals()]


# ------------------------------------------------------------------ the executors against the reference
@pytest.mark.parametrize("b,h,w", CASES)
def test_residuals_and_controlled_output_against_the_reference(unet, cnet, masters, b, h, w):
    sd, cn_sd, ms = masters
    x, s, ctx, hint = case(b, h, w)
    got = branch(cnet, x, s, ctx, hint)
    want = R.control_residuals(cn_sd, CFG, ms, x, s, ctx, hint)
    assert len(got) == len(want) == cnet.residual_count + 1
    errs = [rel_l2(g, r) for g, r in zip(got, want)]
    print("residual rel-L2:", ["%.2e" % e for e in errs])
    assert all(tuple(g.shape) == tuple(r.shape) for g, r in zip(got, want))
    assert max(errs) < UNET_TOL, errs                              # each residual on its own
    unet.set_context(ctx)
    for strength in (1.0, 0.6):
        out = unet.forward(x.to(DEV), s.to(DEV), control=cnet.control(strength)).cpu()
        ref = R.apply_model(sd, CFG, ms, x, s, ctx, cn_sd, hint, strength)
        print("controlled output rel-L2 at strength", strength, "%.2e" % rel_l2(out, ref))
        assert rel_l2(out, ref) < UNET_TOL, (strength, rel_l2(out, ref))
    plain = unet.forward(x.to(DEV), s.to(DEV)).cpu()
    assert rel_l2(out, plain) > 10 * UNET_TOL                      # and control really moved it
    eps = unet.forward(x.to(DEV), s.to(DEV), control=cnet.control(1.0), eps_only=True).cpu()
    assert rel_l2(eps, R.apply_model(sd, CFG, ms, x, s, ctx, cn_sd, hint, 1.0, eps_only=True)) < UNET_TOL


@pytest.mark.parametrize("b,h,w", CASES)
def test_strength_zero_and_a_null_control_are_the_plain_forwards_bits(unet, cnet, b, h, w):
    x, s, ctx, hint = case(b, h, w, ctx_rows=2 * b)
    xd, sd_ = x.to(DEV), s.to(DEV)
    x2, s2 = torch.cat([xd, xd]).contiguous(), torch.cat([sd_, sd_]).contiguous()
    cnet.set_context(ctx)
    cnet.set_hint(hint)
    cnet.forward(x2, s2)
    unet.set_context(ctx)
    plain, n_plain = unet.forward(x2, s2).clone(), unet.last_launches
    assert same_bits(unet.forward(x2, s2, control=cnet.control(0.0)), plain) and unet.last_launches == n_plain
    assert same_bits(unet.forward(x2, s2, control=None), plain) and unet.last_launches == n_plain
    assert not same_bits(unet.forward(x2, s2, control=cnet.control(1.0)), plain) and unet.last_launches == n_plain + 1      # ONE launch more
    pair, n_pair = unet.forward_pair(xd, sd_).clone(), unet.last_launches
    assert same_bits(unet.forward_pair(xd, sd_, control=cnet.control(0.0)), pair) and unet.last_launches == n_pair
    assert same_bits(unet.forward_pair(xd, sd_, control=None), pair) and unet.last_launches == n_pair
    assert not same_bits(unet.forward_pair(xd, sd_, control=cnet.control(1.0)), pair) and unet.last_launches == n_pair + 1


def test_all_zero_zero_convolutions_are_the_plain_forwards_bits(unet):
    from lightdiffusion_amd.controlnet import MI355XControlNet
    zero = lambda name, shape: (torch.zeros(shape) if name.startswith(("zero_convs.", "middle_block_out.")) else W.synth_controlnet_tensor(name, shape))
    cn = MI355XControlNet(CFG, zero, max_batch=2, max_hw=(8, 24))
    x, s, ctx, hint = case(2, 8, 24)
    res = branch(cn, x, s, ctx, hint)
    assert all(float(r.abs().max()) == 0.0 for r in res)
    unet.set_context(ctx)
    plain = unet.forward(x.to(DEV), s.to(DEV)).clone()
    assert same_bits(unet.forward(x.to(DEV), s.to(DEV), control=cn.control(1.0)), plain)


@pytest.mark.parametrize("b,h,w", CASES)
def test_pair_forms_equal_the_plain_forms_on_duplicated_inputs(unet, cnet, b, h, w):
    x, s, ctx, hint = case(b, h, w, ctx_rows=2 * b)
    xd, sd_ = x.to(DEV), s.to(DEV)
    x2, s2 = torch.cat([xd, xd]).contiguous(), torch.cat([sd_, sd_]).contiguous()
    cnet.set_context(ctx)
    cnet.set_hint(hint)
    cnet.forward(x2, s2)
    full = cnet.residuals()
    unet.set_context(ctx)
    out_full = unet.forward(x2, s2, control=cnet.control(1.0)).clone()
    cnet.forward_pair(xd, sd_)
    pair = cnet.residuals()
    assert all(p.shape == f.shape and rel_l2(p.float().cpu(), f.float().cpu()) < 1e-3 for p, f in zip(pair, full))
    assert not torch.equal(pair[-1][:b], pair[-1][b:])             # the cond half saw the other context
    unet_out = unet.forward_pair(xd, sd_, control=cnet.control(1.0))
    assert rel_l2(unet_out.cpu(), out_full.cpu()) < 1e-3


def test_a_wrong_count_shape_or_batch_is_refused_and_writes_nothing(unet, cnet):
    x, s, ctx, hint = case(2, 8, 24)
    xd, sd_ = x.to(DEV), s.to(DEV)
    cnet.set_context(ctx)
    cnet.set_hint(hint)
    cnet.forward(xd, sd_)
    unet.set_context(ctx)
    out = torch.full_like(xd, 7.0)

    def status(ctl, xx=xd):
        with pytest.raises(LDError) as e:
            unet.forward(xx, sd_, control=ctl, out=out)
        assert bool((out == 7.0).all())
        return e.value.status

    ctl = cnet.control(1.0)
    ctl.count -= 1
    assert status(ctl) == ERR_SHAPE
    ctl = cnet.control(1.0)
    ctl.c[3] += 8
    assert status(ctl) == ERR_SHAPE
    ctl = cnet.control(1.0)
    ctl.h[ctl.count] += 1                                          # the middle one
    assert status(ctl) == ERR_SHAPE
    ctl = cnet.control(1.0, r_n=3)                                 # does not divide the batch of 2
    assert status(ctl) == ERR_SHAPE
    assert status(cnet.control(1.0), torch.zeros(2, 4, 16, 16, device=DEV)) == ERR_SHAPE      # residuals of another latent size
    ctl = cnet.control(1.0)
    ctl.residual[5] = None
    assert status(ctl) == ERR_ARG
    # ... and the control branch refuses a latent that is not its hint's, a UNet handle refuses a control call
    with pytest.raises(LDError) as e:
        cnet.forward(torch.zeros(2, 4, 8, 8, device=DEV), sd_)
    assert e.value.status == ERR_SHAPE
    from lightdiffusion_amd._lib import lib
    assert lib().ld_controlnet_forward(unet._h, xd.data_ptr(), sd_.data_ptr(), 2, 8, 24, 0, None) == ERR_ARG
    assert lib().ld_unet_forward(cnet._h, xd.data_ptr(), sd_.data_ptr(), out.data_ptr(), 2, 8, 24, 0, None, None) == ERR_ARG


def test_loaded_state_dict_reads_back(cnet):
    """ControlNetLoader's path: a state dict under the control_model. prefix, the configuration read from its shapes"""
    sd = {"control_model." + k: v for k, v in R.synth_state_dict(CFG).items()}
    cn = N.ControlNetLoader(DEV, max_hw=(8, 8)).load_controlnet(sd)[0]
    assert cn.control_model.param_shapes() == W.controlnet_param_shapes(CFG) == cnet.param_shapes()
    for name in ("zero_convs.3.0.weight", "input_hint_block.4.weight", "middle_block_out.0.bias"):
        assert torch.equal(cn.control_model.read_param(name).cpu(), sd["control_model." + name].half())


# ------------------------------------------------------------------ the sampler
TOKS = [[(49406, 1.0)] + [(320, 1.0)] * 3 + [(49407, 1.0)] * 73]
NEG = [[(49406, 1.0)] + [(1125, 1.0)] * 2 + [(49407, 1.0)] * 74]
STEPS, SCALE, SEED = 4, 3.0, 11


@pytest.fixture(scope="module")
def tiny():
    model, clip, vae = N.load_synthetic(DEV, max_batch=2, max_hw=(8, 16), tiny=True)
    enc = lambda t: [[c, {"pooled_output": p}] for c, p in [clip.encode_from_tokens(t, return_pooled=True)]]
    control_net = N.load_synthetic_controlnet(DEV, max_batch=2, max_hw=(8, 16), tiny=True)
    image = torch.rand(1, 64, 128, 3, generator=torch.Generator().manual_seed(9))
    return model, enc(TOKS), enc(NEG), control_net, image


def run(model, pos, neg, b=2, **kw):
    """-> (samples on the host, [(sigma, x before the step (None for the first), denoised)])"""
    latent = torch.randn(b, 4, 8, 16, generator=torch.Generator().manual_seed(5 + b))
    sigmas = S.calculate_sigmas(model.get_model_object("model_sampling"), "normal", STEPS)
    seen, before = [], [None]

    def callback(d):
        seen.append((d["sigma"], before[0], d["denoised"].clone()))
        before[0] = d["x"].clone()
    noise = S.prepare_noise(latent, SEED)
    out = S.sample(model, noise, pos, neg, SCALE, model.load_device, S.ksampler("euler_ancestral"), sigmas, model.model_options, latent_image=latent,
                   callback=callback, seed=SEED, **kw)
    return out.cpu(), seen


def test_sampler_graph_replay_is_eager_launches_and_control_is_applied(tiny):
    model, pos, neg, cn, image = tiny
    cpos = N.ControlNetApply().apply_controlnet(pos, cn, image, 1.0)[0]
    out, seen = run(model, cpos, neg, apply_control=True)
    eager = model.clone()
    eager.model_options["ld_use_graph"] = False
    out_eager, _ = run(eager, cpos, neg, apply_control=True)
    assert same_bits(out, out_eager)
    inert, _ = run(model, cpos, neg)                                # without the keyword the key is inert
    plain, _ = run(model, pos, neg)
    assert same_bits(inert, plain)
    assert rel_l2(out, plain) > 10 * UNET_TOL                       # with it, it is not
    assert len(seen) == STEPS


def test_sampler_step_range_controls_exactly_the_steps_inside_it(tiny):
    model, pos, neg, cn, image = tiny
    unet = model.model_options["model_function_wrapper"]
    ms = model.get_model_object("model_sampling")
    p_on, n_on = N.ControlNetApplyAdvanced().apply_controlnet(pos, neg, cn, image, 1.0, 0.0, 1.0)
    p_rng, n_rng = N.ControlNetApplyAdvanced().apply_controlnet(pos, neg, cn, image, 1.0, 0.0, 0.5)
    _, on = run(model, p_on, n_on, apply_control=True)
    _, off = run(model, pos, neg)
    _, rng = run(model, p_rng, n_rng, apply_control=True)
    lo = ms.percent_to_sigma(0.5)
    inside = [sig >= lo for sig, _, _ in rng]
    assert inside == sorted(inside, reverse=True) and any(inside) and not all(inside), inside
    k = inside.index(False)
    for i in range(k):                                              # inside the range: the always-on run's steps, bit for bit
        assert same_bits(rng[i][2], on[i][2]), i
        assert not same_bits(rng[i][2], off[i][2]), i
    # from the first step outside on, each step is the ORDINARY guided step on the x it was given (the trajectory has left both other runs)
    ctx = torch.cat([neg[0][0].expand(2, -1, -1), pos[0][0].expand(2, -1, -1)]).contiguous().to(DEV)
    probe = p_on[0][1]["control"].copy()
    probe.pre_run(None, ms.percent_to_sigma)
    for i in range(k, STEPS):
        sig, x_before, den = rng[i]
        ts = torch.full((2,), float(sig), device=DEV)
        assert same_bits(den, unet.cfg_denoise(x_before, ts, ctx, SCALE)), i
        assert not same_bits(den, unet.cfg_denoise(x_before, ts, ctx, SCALE, control=probe)), i
    # ... and the first of them starts from the always-on run's x
    assert same_bits(rng[k][1], on[k][1])


def test_sampler_encodes_the_hint_once_and_a_batch_one_hint_serves_batch_two(tiny, monkeypatch):
    from lightdiffusion_amd.controlnet import MI355XControlNet
    model, pos, neg, cn, image = tiny
    calls = []
    set_hint = MI355XControlNet.set_hint
    monkeypatch.setattr(MI355XControlNet, "set_hint", lambda self, img: (calls.append(tuple(img.shape)), set_hint(self, img))[1])
    cpos = N.ControlNetApply().apply_controlnet(pos, cn, image, 1.0)[0]
    out1, _ = run(model, cpos, neg, apply_control=True)
    assert calls == [(1, 3, 64, 128)] and cpos[0][1]["control"].encode_calls == 1         # once for the run's four steps, resized to 8h x 8w
    both = N.ControlNetApply().apply_controlnet(pos, cn, image.expand(2, -1, -1, -1), 1.0)[0]
    out2, _ = run(model, both, neg, apply_control=True)
    assert calls[1:] == [(2, 3, 64, 128)]
    assert same_bits(out1, out2)                                    # sample s reads hint s % 1
    big = N.ControlNetApply().apply_controlnet(pos, cn, torch.rand(1, 96, 192, 3), 1.0)[0]    # another size: resized once
    run(model, big, neg, apply_control=True)
    assert calls[2:] == [(1, 3, 64, 128)]
    three = N.ControlNetApply().apply_controlnet(pos, cn, image.expand(3, -1, -1, -1), 1.0)[0]
    with pytest.raises(ValueError, match="hint batch"):
        run(model, three, neg, apply_control=True)


def test_handle_load_unload_load():
    """tests/test_lifecycle_gpu.py's wrapper pattern for the fifth resident model"""
    from lightdiffusion_amd.controlnet import synthetic_controlnet
    x, s, ctx, hint = case(1, 8, 8)
    results = []
    for _ in range(2):
        m = synthetic_controlnet(CFG, max_batch=1, max_hw=(8, 8))
        ws, epoch = m.workspace_bytes, m.reserve_epoch
        assert ws > 0 and tuple(m._reserved[:3]) == (1, 8, 8)
        m.set_context(ctx)                                          # inside the plan: the workspace stays
        assert m.workspace_bytes == ws and m.reserve_epoch == epoch
        m.set_context(torch.cat([ctx, ctx]))                        # a larger call re-reserves
        assert tuple(m._reserved[:3]) == (2, 8, 8) and m.workspace_bytes > ws and m.reserve_epoch == epoch + 1
        assert m.hint_shape is None
        with pytest.raises(LDError):                                # no hint since the workspace moved
            m.forward(torch.cat([x, x]).to(DEV), torch.cat([s, s]).to(DEV))
        results.append(branch(m, x, s, ctx, hint))
        torch.cuda.synchronize()
        m.__del__()
        assert not m._h.value
        m.__del__()
    assert all(torch.equal(a, b) for a, b in zip(*results))
