"""GPU: masked denoising on the device, on the tiny synthetic model (latents 1x4x8x12 and 2x4x8x12, 4 steps).
  (a) for euler_ancestral, dpmpp_2m_sde (eta = 0) and dpm_adaptive the final samples of the device route (sampling.KSamplerX0Inpaint over the two
      HIP blends) are BITWISE those of a second run in which a test-local wrapper evaluates the two blend expressions in torch around the same
      model; everything else is the same code, so any difference would be the kernels' or the wrapper's;
  (b) with a mask that is 0 on the left half, the kept half of the final latent is latent_image within a bound derived per sampler (below) and
      the other half is redrawn — THE test of the feature: where the keyword is swallowed the kept half is redrawn too;
  (c) nodes.inpaint end to end; one Detailer segment with apply_noise_mask=True; the guided step of the masked route replays the graph captured
      for the unmasked one; DifferentialDiffusion's device-side threshold is its host-side one.

THE BOUNDS OF (b), per element, u = 2^-24 (fp32 round to nearest), L = latent_image, x_last = the returned latent.  The sampler works on
L_s = L * 0.18215 (process_latent_in) and returns samples / 0.18215 (a product, and a division that may be a reciprocal and a product): at most
three roundings, 3 u |L| between them, in every case.
  euler_ancestral   the last step, to sigma = 0, computes x + (x - den) / sigma * (-sigma): three fp32 roundings on values of that size; with the
                    blend's den = L_s there the bound is 8 u (|x_last| + |L|) (the issue's; it covers the scaling's roundings as well).
  dpmpp_2m_sde      the last step is x = denoised, and the blend leaves denoised = den * 0 + L_s * 1 = L_s exactly: only the scaling's
                    roundings remain, 3 u |L| <= 2 u (|x_last| + |L|).
  dpm_adaptive      stops at sigma_end > 0 and never steps to 0.  In the kept half the model's answer is L_s at every evaluation, so the solver's
                    eps = (x - L_s) / sigma is one constant e = (x0 - L_s) / sigma_0 (the run's noise; times sqrt(1 + sigma^2) / sigma when the run
                    starts at sigma_max), which DPM-Solver integrates exactly: the kept half ends at L_s + sigma_end e, NOT at L_s — that is what
                    the sampler does to every latent, masked or not.  The test holds x_last to (L_s + sigma_end e) / 0.18215 within a running
                    bound on y = (x - L_s) / sigma, which is e but for rounding.  One accepted step of width h = log(sigma_s / sigma_t) moves y
                    by at most
                        360 exp(2 h) u (|e| + |L_s| / sigma_t)
                    counted as follows.  A new x or stage point is x - c eps (- d (eps' - eps)); in units of y at a point of sigma_p it errs by
                    (i) 24 u (sigma_s / sigma_p - 1) |e| for the product c eps: c = sigma_s - sigma_p comes from fp32 exp / expm1 on the host
                    (<= 16 u), eps = (x - L_s) * (1 / sigma) has a subtraction, a reciprocal and a product (3 u), the product c eps one more,
                    rounded up; (ii) 2 u (|L_s| / sigma_p + |e|) for the subtractions that finish the point; (iii) the weight of its
                    difference term times the error of that difference, which is the error of the stage point behind it plus 2 * 24 u |e|.
                    The weights over sigma are 2 (expm1(2h/3) / (2h/3) - 1) <= 2 exp(2h/3) for the second stage point and
                    1.5 (expm1(h) / h - 1) <= 1.5 exp(h) for x_high, and sigma_s / sigma_p - 1 <= exp(h).  Nesting (i)-(iii) from the first stage
                    point to x_high and bounding every exponential by exp(2h):
                        |e| part      24 + 2 + 1.5 (48 + 2 + 24 + 2 (48 + 2 + 24)) = 359
                        |L_s| part    2 + 1.5 (2 + 2 * 2) = 11
                    both below 360.  An error already in y is carried unchanged (every eps of the step sees it alike and the difference terms
                    cancel it).  The bound is sigma_end times the sum over the accepted steps the callback saw, plus the start's 2 u (|L_s| +
                    sigma_0 |e|) carried as y, divided by 0.18215, plus 4 u (|x_last| + |L|) for the scaling on both sides.  (Measured: the
                    worst element sits below a hundredth of it, and it stays some hundreds of times below the sigma_end e it isolates.)"""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detailer_standins as DS                                 # noqa: E402
from test_detailer_cpu import flow_segs                        # noqa: E402
from lightdiffusion_amd import detailer as D                   # noqa: E402
from lightdiffusion_amd import nodes as N                      # noqa: E402
from lightdiffusion_amd import pipeline as P                   # noqa: E402
from lightdiffusion_amd import sampling as S                   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOKS = [[(49406, 1.0)] + [(320, 1.0)] * 3 + [(49407, 1.0)] * 73]
NEG = [[(49406, 1.0)] + [(1125, 1.0)] * 2 + [(49407, 1.0)] * 74]
SAMPLERS = ["euler_ancestral", "dpmpp_2m_sde", "dpm_adaptive"]
STEPS, CFG, SEED, U = 4, 3.0, 11, 2.0 ** -24
SCALE = S.LATENT_SCALE


@pytest.fixture(scope="module")
def tiny():
    model, clip, vae = N.load_synthetic(DEV, max_batch=2, max_hw=(8, 12), tiny=True)
    enc = lambda t: [[c, {"pooled_output": p}] for c, p in [clip.encode_from_tokens(t, return_pooled=True)]]
    return model, clip, vae, enc(TOKS), enc(NEG)


def latent_of(b):
    return torch.randn(b, 4, 8, 12, generator=torch.Generator().manual_seed(5 + b))


def left_half_mask():
    m = torch.ones(8, 12)
    m[:, :6] = 0.0
    return m


KEPT = (slice(None), slice(None), slice(None), slice(0, 6))
DRAWN = (slice(None), slice(None), slice(None), slice(6, 12))


def run(tiny, sampler, latent, mask=None, apply=True, callback=None):
    """sampling.sample on the tiny model, 4 steps of the normal schedule (dpmpp_2m_sde with eta = 0) -> the samples on the host"""
    model, _, _, pos, neg = tiny
    sigmas = S.calculate_sigmas(model.get_model_object("model_sampling"), "normal", STEPS)
    ks = S.ksampler(sampler, {"eta": 0.0} if sampler == "dpmpp_2m_sde" else None, {"apply_denoise_mask": True} if apply else None)
    out = S.sample(model, S.prepare_noise(latent, SEED), pos, neg, CFG, model.load_device, ks, sigmas, model.model_options, latent_image=latent,
                   denoise_mask=mask, callback=callback, seed=SEED)
    return out.cpu()


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


class TorchInpaint:
    """sampling.KSamplerX0Inpaint with the two blends as torch expressions, operation by operation in fp32 on the device"""
    calls = 0

    def __init__(self, model_wrap, sigmas, noise, latent_image, denoise_mask):
        self.inner_model, self.sigmas, self.noise, self.latent_image, self.denoise_mask = model_wrap, sigmas, noise, latent_image, denoise_mask

    def __call__(self, x, sigma, model_options=None, seed=None, **_unused):
        TorchInpaint.calls += 1
        m = self.denoise_mask
        if "denoise_mask_function" in model_options:
            m = model_options["denoise_mask_function"](sigma, m, extra_options={"model": self.inner_model, "sigmas": self.sigmas})
        x_in = x * m + (self.noise * sigma.view(-1, 1, 1, 1) + self.latent_image) * (1.0 - m)
        out = self.inner_model(x_in, sigma, model_options=model_options, seed=seed)
        return out * m + self.latent_image * (1.0 - m)


# ------------------------------------------------------------------ (a)
@pytest.mark.parametrize("b", [1, 2])
@pytest.mark.parametrize("sampler", SAMPLERS)
def test_device_route_is_the_torch_wrappers_bits(tiny, monkeypatch, sampler, b):
    g = torch.Generator().manual_seed(3)
    mask = torch.rand(b, 64, 96, generator=g)                       # on the pixel grid, a mask per sample; exact 0 and 1 inside
    mask[:, :24] = 0.0
    mask[:, 40:] = 1.0
    lat = latent_of(b)
    got = run(tiny, sampler, lat, mask)
    monkeypatch.setattr(S, "KSamplerX0Inpaint", TorchInpaint)
    TorchInpaint.calls = 0
    want = run(tiny, sampler, lat, mask)
    assert TorchInpaint.calls >= STEPS, "the second run went through the test's wrapper"
    assert same_bits(got, want)
    assert torch.isfinite(got).all() and not same_bits(got, run(tiny, sampler, lat, mask, apply=False)), "and the mask is not inert"


# ------------------------------------------------------------------ (b)
def adaptive_bound(L, noise, sigmas, seen, x_last):
    """the module docstring's bound for dpm_adaptive, and what the kept half ends at: (bound, target), fp64 on the host"""
    ms = S.ModelSampling()
    s0 = float(sigmas[0])
    Ls = (L * SCALE).double()
    x0 = ms.noise_scaling(sigmas[0], noise, L * SCALE, max_denoise=True).double()     # 4 steps of the whole schedule start at sigma_max
    e = (x0 - Ls) / s0
    y_err = 2 * U * (Ls.abs() / s0 + e.abs())
    prev, steps = s0, 0
    for sig in seen:
        if sig == prev:                                                                # a rejected proposal: x did not move
            continue
        h = math.log(prev / sig)
        y_err = y_err + 360.0 * math.exp(2 * h) * U * (e.abs() + Ls.abs() / sig)
        prev, steps = sig, steps + 1
    target = (Ls + prev * e) / SCALE
    bound = prev * y_err / SCALE + 4 * U * (x_last.double().abs() + L.double().abs())
    return bound, target, steps, prev


@pytest.mark.parametrize("b", [1, 2])
@pytest.mark.parametrize("sampler", SAMPLERS)
def test_kept_half_is_the_latent_and_the_other_half_is_drawn(tiny, sampler, b):
    L = latent_of(b)
    seen = []
    out = run(tiny, sampler, L, left_half_mask(), callback=lambda d: seen.append(float(d["sigma"])))
    assert tuple(out.shape) == tuple(L.shape) and torch.isfinite(out).all()
    size = out.double().abs() + L.double().abs()
    if sampler == "dpm_adaptive":
        sigmas = S.calculate_sigmas(S.ModelSampling(), "normal", STEPS)
        bound, target, steps, s_end = adaptive_bound(L, S.prepare_noise(L, SEED), sigmas, seen, out)
        assert abs(s_end / float(sigmas[-2]) - 1.0) < 1e-4 and steps >= 3
        err = (out.double() - target).abs()
        print(f"{sampler} b={b}: {steps} accepted steps of {len(seen)}, sigma_end {s_end:.5f}; kept half vs L + sigma_end e: worst error / bound "
              f"{float((err / bound)[KEPT].max()):.3f}, worst error {float(err[KEPT].max()):.3e}")
        assert bool((err <= bound)[KEPT].all())
    else:
        k = 8 if sampler == "euler_ancestral" else 2
        err = (out.double() - L.double()).abs()
        print(f"{sampler} b={b}: kept half vs latent_image: worst error / ({k} u (|x_last| + |latent|)) {float((err / (k * U * size))[KEPT].max()):.3f}")
        assert bool((err <= k * U * size)[KEPT].all())
    assert float((out - L)[DRAWN].abs().mean()) > 0.05, "the other half is redrawn"
    free = run(tiny, sampler, L, left_half_mask(), apply=False)
    assert float((free - L)[KEPT].abs().mean()) > 0.05, "without the option the mask is inert and the kept half is redrawn too"


def test_ksampler2_keeps_the_masked_half(tiny):
    """The public route: SetLatentNoiseMask, then KSampler2(apply_noise_mask=True) with euler_ancestral; the issue's bound.  Off, the node's
    result is that of a latent without a mask, bit for bit."""
    model, _, _, pos, neg = tiny
    L = latent_of(2)
    lat = N.SetLatentNoiseMask().set_mask({"samples": L}, left_half_mask())[0]
    args = (model, SEED, STEPS, CFG, "euler_ancestral", "normal", pos, neg)
    out = N.KSampler2().sample(*args, lat, apply_noise_mask=True)[0]
    assert out["noise_mask"] is lat["noise_mask"] and out["samples"].device.type == "cpu"
    x = out["samples"]
    err = (x.double() - L.double()).abs()
    assert bool((err <= 8 * U * (x.double().abs() + L.double().abs()))[KEPT].all())
    assert float((x - L)[DRAWN].abs().mean()) > 0.05
    off = N.KSampler2().sample(*args, lat)[0]["samples"]
    assert same_bits(off, N.KSampler2().sample(*args, {"samples": L})[0]["samples"])
    assert float((off - L)[KEPT].abs().mean()) > 0.05


# ------------------------------------------------------------------ (c)
@pytest.mark.parametrize("b", [1, 2])
def test_inpaint_end_to_end(tiny, b):
    model, clip, vae, _, _ = tiny
    g = torch.Generator().manual_seed(9)
    image = torch.rand(b, 64, 96, 3, generator=g)
    mask = torch.zeros(64, 96)
    mask[16:48, 32:80] = 1.0
    torch.manual_seed(2)
    out = N.inpaint(model, clip, vae, image, mask, TOKS, NEG, seed=SEED, steps=STEPS, cfg=CFG, sampler_name="euler_ancestral", scheduler="normal")
    assert tuple(out.shape) == (b, 64, 96, 3) and out.dtype == torch.float32 and out.device.type == "cpu" and torch.isfinite(out).all()
    assert float(out.min()) >= 0.0 and float(out.max()) <= 1.0
    torch.manual_seed(2)
    ones = N.inpaint(model, clip, vae, image, torch.ones(64, 96), TOKS, NEG, seed=SEED, steps=STEPS, cfg=CFG, sampler_name="euler_ancestral",
                     scheduler="normal")
    assert not torch.equal(out, ones), "the mask reaches the sampler"


def test_masked_route_replays_the_captured_graph(tiny, monkeypatch):
    model = tiny[0]
    unet = model.model_options["model_function_wrapper"]
    L = latent_of(2)
    run(tiny, "euler_ancestral", L, None, apply=False)                       # the unmasked route captures (or has captured) this shape's step
    key = (2, 8, 12, CFG, True)
    den = unet._denoisers[key]
    graph = den._graph
    assert isinstance(den, P.CFGDenoiser) and graph is not None
    captures, launches = [], []
    capture, launch = P.GraphedBody._capture, P.GraphedBody.launch
    monkeypatch.setattr(P.GraphedBody, "_capture", lambda self: (captures.append(self), capture(self))[1])
    monkeypatch.setattr(P.GraphedBody, "launch", lambda self: (launches.append(self), launch(self))[1])
    run(tiny, "euler_ancestral", L, left_half_mask())
    assert unet._denoisers[key] is den and den._graph is graph, "the same denoiser and the same graph object after a masked run of the shape"
    assert captures == [] and launches == [den._run] * STEPS, "every guided step of the masked route was one replay of it"


def test_differential_diffusion_on_the_device_is_the_host_route(tiny):
    """forward with sigma on the device (no host read of it) gives the mask of forward with the same sigma on the host"""
    model = tiny[0]
    ms = model.get_model_object("model_sampling")
    guider = S.CFGGuider(model)
    guider.inner_model = model.model
    dd = D.DifferentialDiffusion()
    ramp = torch.linspace(0.0, 1.0, 96).view(1, 1, 8, 12).contiguous()
    for sigmas in (S.calculate_sigmas(ms, "normal", 12), S.calculate_sigmas(ms, "karras", 9)):
        eo = {"model": guider, "sigmas": sigmas}
        opened = []
        for s in sigmas[:-1]:
            sig = torch.full((2,), float(s))
            host = dd.forward(sig, ramp, eo)
            got = dd.forward(sig.to(DEV), ramp.to(DEV), eo)
            assert got.is_cuda and same_bits(got.cpu(), host)
            opened.append(int(host.sum()))
        assert opened == sorted(opened) and opened[0] <= 1 and opened[-1] > 48, "the mask opens up as sigma falls"


def test_detailer_applies_the_noise_mask(tiny, monkeypatch):
    """One 64 x 64 segment, apply_noise_mask=True, noise_mask_feather=4: DifferentialDiffusion.forward is called once per model call, the result
    differs from the option-off run inside the crop, and outside the crop the canvas is the input's bits.  (The option-off run against the
    goldens: tests/test_detailer_gpu.py.)"""
    model, clip, vae, pos, neg = tiny
    image, (shape, items) = flow_segs()
    seg = items[2]
    x1, y1, x2, y2 = seg.crop_region
    assert (x2 - x1, y2 - y1) == (64, 64)
    p = DS.flow_params()
    unet = model.model_options["model_function_wrapper"]
    counts = {"forward": 0, "model": 0}
    forward, cfg_denoise = D.DifferentialDiffusion.forward, unet.cfg_denoise

    def counting_forward(self, sigma, mask, extra_options):
        counts["forward"] += 1
        assert sigma.is_cuda and mask.is_cuda and tuple(mask.shape) == (1, 1, 8, 8)
        out = forward(self, sigma, mask, extra_options)
        assert set(out.unique().tolist()) <= {0.0, 1.0}
        return out

    def counting_model(*a, **kw):
        counts["model"] += 1
        return cfg_denoise(*a, **kw)
    monkeypatch.setattr(D.DifferentialDiffusion, "forward", counting_forward)
    monkeypatch.setattr(unet, "cfg_denoise", counting_model, raising=False)

    def doit(**kw):
        torch.manual_seed(3)
        return N.DetailerForEach().doit(image, (shape, [seg]), model, clip, vae, p["guide_size"], p["guide_size_for_bbox"], p["max_size"], p["seed"], STEPS,
                                        p["cfg"], p["sampler_name"], p["scheduler"], pos, neg, p["denoise"], p["feather"], p["noise_mask"],
                                        p["force_inpaint"], "", noise_mask_feather=4, **kw)[0]
    off = doit()
    assert counts == {"forward": 0, "model": STEPS}, "off: the function is installed and never called"
    assert "denoise_mask_function" not in model.model_options
    on = doit(apply_noise_mask=True)
    assert counts == {"forward": STEPS, "model": 2 * STEPS}, "on: once per model call"
    assert "denoise_mask_function" not in model.model_options, "the function went onto a clone"
    outside = np.ones(DS.FLOW_SHAPE, bool)
    outside[y1:y2, x1:x2] = False
    bits = lambda t: t.numpy().view(np.uint32)
    for res in (on, off):
        assert tuple(res.shape) == tuple(image.shape) and np.array_equal(bits(res[0])[outside], bits(image[0])[outside]), "outside the crop: untouched"
        assert not torch.equal(res[0, y1:y2, x1:x2], image[0, y1:y2, x1:x2])
    assert not torch.equal(on[0, y1:y2, x1:x2], off[0, y1:y2, x1:x2]), "inside the crop the option changes the redraw"
