"""GPU: regional conditioning on the device, on the tiny synthetic model (latents B x 4 x 16 x 24, B in {1, 2}; 4 steps; euler_ancestral and
dpmpp_2m_sde with eta = 0).
  (a) the final samples of the device route (ops.regional_gather / ops.regional_combine around the eager UNet calls) are BITWISE those of a
      second run in which both ops are replaced by tests/regional_ref.py's torch expressions (evaluated in fp32 on the host, where every
      product, sum and division is IEEE); everything else is the same code.  And they differ from the option-off run: the keys are not inert;
  (b) two positive entries with the SAME prompt and complementary 0 / 1 masks over the whole latent: the UNet call is the same batch and gives
      the same bits, and out * 1 / (1e-37 + 1) and (out + out) / 2 are both out — the option-on result is the option-off result wherever the
      UNet gave the two identical rows the same bits (the test's docstring says where it does not, and why that is not asserted);
  (c) locality: with positive = [whole P0, area entry P1], replacing P1's prompt changes one sampling_function output inside the area only;
  (d) the nodes end to end; option off is today's bits for keyed conditioning; option on with unkeyed single conditioning is today's bits and
      replays the captured graph with no new capture; a run with a step range reads sigma on the host once per step, a run without one never;
      with apply_noise_mask as well the kept half is still the latent (tests/test_inpaint_gpu.py's bounds)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import regional_ref as R                                       # noqa: E402
from lightdiffusion_amd import nodes as N                      # noqa: E402
from lightdiffusion_amd import ops                             # noqa: E402
from lightdiffusion_amd import pipeline as P                   # noqa: E402
from lightdiffusion_amd import sampling as S                   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W = 16, 24
STEPS, CFG, SEED, U = 4, 3.0, 11, 2.0 ** -24
SAMPLERS = ["euler_ancestral", "dpmpp_2m_sde"]
A1, A2 = (8, 16, 0, 8), (16, 8, 0, 4)              # two shapes; they overlap in rows 0..7, columns 8..11, inside A1's left and A2's right ramp
same_bits = R.same_bits


def toks(word):
    return [[(49406, 1.0)] + [(word, 1.0)] * 3 + [(49407, 1.0)] * 73]


@pytest.fixture(scope="module")
def tiny():
    model, clip, vae = N.load_synthetic(DEV, max_batch=6, max_hw=(H, W), tiny=True)
    enc = lambda t: [[c, {"pooled_output": p}] for c, p in [clip.encode_from_tokens(t, return_pooled=True)]]
    prompts = {k: enc(toks(w)) for k, w in (("p0", 320), ("p1", 530), ("p2", 1125), ("neg", 2368))}
    return model, prompts


def latent_of(b):
    return torch.randn(b, 4, H, W, generator=torch.Generator().manual_seed(5 + b))


def frac_mask(seed, *shape):
    return torch.randint(0, 65, shape, generator=torch.Generator().manual_seed(seed)).float() / 64.0


def keyed(c, **keys):
    return [[t, dict(d, **keys)] for t, d in c]


def mixed(prompts, b):
    """a whole entry, two overlapping areas of different shapes (one at strength 0.5), a fractional mask on the pixel grid, per sample"""
    pos = prompts["p0"] + keyed(prompts["p1"], area=A1, strength=1.0) + keyed(prompts["p2"], area=A2, strength=0.5) + \
        N.ConditioningSetMask().append(prompts["p1"], frac_mask(3, b, 8 * H, 8 * W), "default", 0.75)[0]
    return pos, prompts["neg"]


def run(model, sampler, pos, neg, b, latent=None, **kw):
    lat = {"samples": latent_of(b) if latent is None else latent}
    lat.update(kw.pop("extra", {}))
    torch.manual_seed(3)                                        # euler_ancestral draws its step noise on the host's global generator
    ks = N.KSampler2()
    if sampler == "dpmpp_2m_sde":                               # eta = 0 through the sampler's own options: the node has no argument for it
        sigmas = S.calculate_sigmas(model.get_model_object("model_sampling"), "normal", STEPS)
        out = S.sample(model, S.prepare_noise(lat["samples"], SEED), pos, neg, CFG, model.load_device,
                       S.ksampler(sampler, {"eta": 0.0}, {"apply_denoise_mask": True} if kw.get("apply_noise_mask") else None), sigmas,
                       model.model_options, latent_image=lat["samples"], denoise_mask=lat.get("noise_mask") if kw.get("apply_noise_mask") else None,
                       seed=SEED, apply_cond_areas=kw.get("apply_cond_areas", False))
        return out.cpu()
    return ks.sample(model, SEED, STEPS, CFG, sampler, "normal", pos, neg, lat, **kw)[0]["samples"]


def host_gather(x, windows, out=None):
    return R.gather(x.cpu(), windows).to(x.device)


def host_combine(outs, entries, cond_scale, shape, out=None):
    host_combine.calls += 1
    return R.combine(outs, entries, cond_scale, shape).to(outs[0].device)


# ------------------------------------------------------------------ (a)
@pytest.mark.parametrize("b", [1, 2])
@pytest.mark.parametrize("sampler", SAMPLERS)
def test_device_route_is_the_torch_expressions_bits(tiny, monkeypatch, sampler, b):
    model, prompts = tiny
    pos, neg = mixed(prompts, b)
    got = run(model, sampler, pos, neg, b, apply_cond_areas=True)
    off = run(model, sampler, pos, neg, b)
    monkeypatch.setattr(ops, "regional_gather", host_gather)
    monkeypatch.setattr(ops, "regional_combine", host_combine)
    host_combine.calls = 0
    want = run(model, sampler, pos, neg, b, apply_cond_areas=True)
    assert host_combine.calls == STEPS, "the second run went through the test's expressions, once per step"
    assert torch.isfinite(got).all() and same_bits(got, want)
    assert not torch.equal(got, off) and float((got - off).abs().mean()) > 1e-3, "and the keys are not inert"


# ------------------------------------------------------------------ (b)
def complementary(prompts):
    m = (torch.rand(H, W, generator=torch.Generator().manual_seed(4)) > 0.5).float()
    return m, keyed(prompts["p0"], mask=m[None]) + keyed(prompts["p0"], mask=(1.0 - m)[None])


@pytest.mark.parametrize("b", [1, 2])
def test_identical_prompts_under_complementary_masks_are_the_option_off_bits(tiny, monkeypatch, b):
    """One guided step, option off and on, on the same lists.  The UNet call is the same: the same batch, the same sigmas, the same context
    rows, and the same bits come back.  Off, the two positive answers a, b are averaged; on, the 0 / 1 masks select between them:
    u + (select(m, a, b) - u) * scale, bit for bit.  out * 1 / (1e-37 + 1) and (out + out) / 2 are both out, so wherever the UNet gave the two
    positive rows — the same latent, the same prompt — the same bits, on IS off, and that is asserted element by element.
    It is not asserted for whole tensors or whole runs, because the premise a == b is the UNet executor's to keep and it does not always: its
    tile and chunk rounding can follow a row's position in the batch and what the workspaces were reserved for (existing behaviour, none of
    this feature's code).  Measured on the tiny model at 16 x 24: on a fresh model the batch [N, P, P] of one latent has equal P rows, that
    of two latents has not (max |a - b| 0.0085 at |out| up to 13; equal again at 8 x 16 and 64 x 64); after batches of two latents have run
    on the model the rows of one latent differ too (in this module's order the two rows agree at 223 of 1536 elements for one latent, at 1726
    of 3072 for two: printed below).  Where a != b, (a + b) / 2 is neither, and a 4-step run ends ~1e-4 (relative) apart."""
    model, prompts = tiny
    m, pos = complementary(prompts)
    unet = model.model_options["model_function_wrapper"]
    seen = []
    forward, sync = unet.forward, unet._sync_context

    def recording_forward(x, sigma, *a, **kw):
        out = forward(x, sigma, *a, **kw)
        seen[-1] += [x.clone(), sigma.clone(), out.clone()]
        return out
    monkeypatch.setattr(unet, "forward", recording_forward, raising=False)
    monkeypatch.setattr(unet, "_sync_context", lambda ctx, *a, **kw: (seen.append([ctx.clone()]), sync(ctx, *a, **kw))[1], raising=False)
    x, sigma = latent_of(b) * 3.0, torch.full((b,), 2.5)
    inner = model.patch_model()
    conv = lambda c: [dict(d, cross_attn=d["cross_attn"].to(DEV)) for d in S.convert_cond(c)]
    opts = lambda **kw: {k: v for k, v in dict(model.model_options, **kw).items() if k != "_ld_ctx_cache"}
    off = S.sampling_function(inner, x.to(DEV), sigma.to(DEV), conv(prompts["neg"]), conv(pos), CFG, opts()).cpu()
    p, n = S.process_conds(conv(pos), conv(prompts["neg"]), x.shape, torch.device(DEV), inner.model_sampling)
    on = S.sampling_function(inner, x.to(DEV), sigma.to(DEV), n, p, CFG, opts(ld_cond_areas=True)).cpu()
    assert len(seen) == 2 and all(len(s) == 4 for s in seen), "one eager UNet call each"
    for got, want in zip(seen[1], seen[0]):
        assert same_bits(got.float().cpu(), want.float().cpu()), "context rows, latent batch, sigmas and the UNet's answer: the same"
    u, first, second = seen[0][3].cpu().chunk(3)                 # batch order [uncond, the second positive, the first positive]
    assert same_bits(off, u + ((torch.stack([first, second]).sum(0) / 2.0) - u) * CFG)
    sel = torch.where(m.bool(), second, first)                   # the first positive carries m, and it was batched last
    assert same_bits(on, u + (sel - u) * CFG)
    agree = first.view(torch.int32) == second.view(torch.int32)
    print(f"b={b}: the UNet gave the two positive rows the same bits at {int(agree.sum())} of {agree.numel()} elements")
    assert torch.equal(on.view(torch.int32)[agree], off.view(torch.int32)[agree]), "where a == b the option-on result is the option-off result"
    # elsewhere: select(a, b) and (a + b) / 2 lie |a - b| / 2 apart, times the scale, plus the roundings of the two mixes (a few ulp of the
    # largest term, scale * (|u| + |a| + |b|))
    size = float((u.abs() + first.abs() + second.abs()).max())
    assert float((on - off).abs().max()) <= 0.5 * CFG * float((first - second).abs().max()) + 8 * U * (1.0 + CFG) * size


# ------------------------------------------------------------------ (c)
def guided_once(model, pos, neg, x, sigma):
    """one sampling_function call as CFGGuider.sample sets it up, option on -> the guided result on the host"""
    inner = model.patch_model()
    conv = lambda c: [dict(d, cross_attn=d["cross_attn"].to(DEV)) for d in S.convert_cond(c)]
    p, n = S.process_conds(conv(pos), conv(neg), x.shape, torch.device(DEV), inner.model_sampling)
    opts = dict(model.model_options, ld_cond_areas=True)
    opts.pop("_ld_ctx_cache", None)
    return S.sampling_function(inner, x.to(DEV), sigma.to(DEV), n, p, CFG, opts).cpu()


@pytest.mark.parametrize("b", [1, 2])
def test_an_area_entry_acts_inside_its_area_only(tiny, b):
    model, prompts = tiny
    x, sigma = latent_of(b) * 3.0, torch.full((b,), 2.5)
    h, w, y0, x0 = A1
    with_p1 = guided_once(model, prompts["p0"] + keyed(prompts["p1"], area=A1), prompts["neg"], x, sigma)
    with_p2 = guided_once(model, prompts["p0"] + keyed(prompts["p2"], area=A1), prompts["neg"], x, sigma)
    inside = torch.zeros(b, 4, H, W, dtype=torch.bool)
    inside[:, :, y0:y0 + h, x0:x0 + w] = True
    assert torch.isfinite(with_p1).all() and same_bits(with_p1[~inside], with_p2[~inside]), "outside the area: the same bits"
    assert float((with_p1 - with_p2)[inside].abs().mean()) > 1e-4, "inside it the prompt matters"
    assert same_bits(with_p1, guided_once(model, prompts["p0"] + keyed(prompts["p1"], area=A1), prompts["neg"], x, sigma)), "and a call repeats"


# ------------------------------------------------------------------ (d)
def test_nodes_end_to_end(tiny):
    model, prompts = tiny
    m = torch.zeros(8 * H, 8 * W)
    m[:, : 4 * W] = 1.0
    left = N.ConditioningSetMask().append(prompts["p1"], m, "default", 1.0)[0]
    right = N.ConditioningSetMask().append(prompts["p2"], 1.0 - m, "mask bounds", 0.5)[0]
    ranged = N.ConditioningSetTimestepRange().set_range(N.ConditioningSetArea().append(prompts["p0"], 128, 64, 32, 0, 0.75)[0], 0.0, 0.6)[0]
    pos = N.ConditioningCombine().combine(N.ConditioningCombine().combine(left, right)[0], ranged)[0]
    assert len(pos) == 3 and "mask" not in prompts["p1"][0][1]
    lat = {"samples": latent_of(2)}
    args = (model, SEED, STEPS, CFG, "euler_ancestral", "normal", pos, prompts["neg"], lat)
    torch.manual_seed(3)
    on = N.KSampler2().sample(*args, apply_cond_areas=True)[0]["samples"]
    torch.manual_seed(3)
    off = N.KSampler2().sample(*args)[0]["samples"]
    assert on.device.type == "cpu" and tuple(on.shape) == (2, 4, H, W) and torch.isfinite(on).all()
    assert float((on - off).abs().mean()) > 1e-3
    assert "ld_cond_areas" not in model.model_options


@pytest.mark.parametrize("sampler", SAMPLERS)
def test_option_off_is_todays_bits_for_keyed_conditioning(tiny, sampler):
    model, prompts = tiny
    pos, neg = mixed(prompts, 2)
    bare = [[t, {"pooled_output": d["pooled_output"]}] for t, d in pos]
    assert same_bits(run(model, sampler, pos, neg, 2), run(model, sampler, bare, neg, 2))
    assert same_bits(run(model, sampler, pos, neg, 2, apply_cond_areas=False), run(model, sampler, bare, neg, 2))


def test_option_on_with_plain_conditioning_replays_the_captured_graph(tiny, monkeypatch):
    model, prompts = tiny
    unet = model.model_options["model_function_wrapper"]
    pos, neg = prompts["p0"], prompts["neg"]
    off = run(model, "euler_ancestral", pos, neg, 2)                             # captures (or has captured) this shape's guided step
    key = (2, H, W, CFG, True)
    den = unet._denoisers[key]
    graph = den._graph
    assert isinstance(den, P.CFGDenoiser) and graph is not None
    captures, launches = [], []
    capture, launch = P.GraphedBody._capture, P.GraphedBody.launch
    monkeypatch.setattr(P.GraphedBody, "_capture", lambda self: (captures.append(self), capture(self))[1])
    monkeypatch.setattr(P.GraphedBody, "launch", lambda self: (launches.append(self), launch(self))[1])
    boom = lambda *a, **k: (_ for _ in ()).throw(AssertionError("plain conditioning must not gather or combine"))
    monkeypatch.setattr(ops, "regional_gather", boom)
    monkeypatch.setattr(ops, "regional_combine", boom)
    on = run(model, "euler_ancestral", pos, neg, 2, apply_cond_areas=True)
    assert same_bits(on, off), "today's bits"
    assert unet._denoisers[key] is den and den._graph is graph, "the same denoiser and the same graph object"
    assert captures == [] and launches == [den._run] * STEPS, "every guided step was one replay of it"
    assert same_bits(run(model, "euler_ancestral", keyed(pos, strength=1.0), neg, 2, apply_cond_areas=True), off), "strength 1 counts as no key"


def test_sigma_is_read_on_the_host_once_per_step_and_only_for_ranges(tiny, monkeypatch):
    model, prompts = tiny
    reads = []
    host_sigma = S._host_sigma
    monkeypatch.setattr(S, "_host_sigma", lambda t: (reads.append(float(t[0])), host_sigma(t))[1])
    area = keyed(prompts["p1"], area=A1)
    run(model, "euler_ancestral", prompts["p0"] + area, prompts["neg"], 2, apply_cond_areas=True)
    assert reads == [], "no entry carries a range: no host read"
    ranged = N.ConditioningSetTimestepRange().set_range(area, 0.3, 1.0)[0]
    on = run(model, "euler_ancestral", prompts["p0"] + ranged, prompts["neg"], 2, apply_cond_areas=True)
    sigmas = S.calculate_sigmas(model.get_model_object("model_sampling"), "normal", STEPS)
    assert reads == [float(s) for s in sigmas[:-1]], "one read per step, of that step's sigma"
    always = run(model, "euler_ancestral", prompts["p0"] + area, prompts["neg"], 2, apply_cond_areas=True)
    assert torch.isfinite(on).all() and not torch.equal(on, always), "the range took the entry out of the early steps"


@pytest.mark.parametrize("sampler", SAMPLERS)
def test_with_the_noise_mask_as_well_the_kept_half_is_the_latent(tiny, sampler):
    model, prompts = tiny
    pos, neg = mixed(prompts, 2)
    L = latent_of(2)
    m = torch.ones(H, W)
    m[:, : W // 2] = 0.0
    noise_mask = N.SetLatentNoiseMask().set_mask({"samples": L}, m)[0]["noise_mask"]
    out = run(model, sampler, pos, neg, 2, latent=L, extra={"noise_mask": noise_mask}, apply_noise_mask=True, apply_cond_areas=True)
    kept, drawn = (Ellipsis, slice(0, W // 2)), (Ellipsis, slice(W // 2, W))
    k = 8 if sampler == "euler_ancestral" else 2                                 # tests/test_inpaint_gpu.py derives both bounds
    err, size = (out.double() - L.double()).abs(), out.double().abs() + L.double().abs()
    print(f"{sampler}: kept half vs latent: worst error / ({k} u (|x_last| + |latent|)) {float((err / (k * U * size))[kept].max()):.3f}")
    assert torch.isfinite(out).all() and bool((err <= k * U * size)[kept].all())
    assert float((out - L)[drawn].abs().mean()) > 0.05, "the other half is redrawn"
    unmasked = run(model, sampler, pos, neg, 2, latent=L, apply_cond_areas=True)
    assert not torch.equal(out[drawn], unmasked[drawn])
