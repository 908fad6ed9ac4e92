"""CPU: the masked sampler route (sampling.prepare_mask, KSamplerX0Inpaint, the apply_noise_mask keyword) on a toy denoiser, with the samplers'
device operators replaced by their torch arithmetic on the host (test_preview_cpu.host_update_arithmetic) and the two blends on
ops.inpaint_in / ops.inpaint_out_'s own host path.
  * prepare_mask is upstream's resize-and-repeat, one channel kept;
  * the wrapper asks the denoise-mask function once per model call, with sigma, the prepared mask and extra_options {"model", "sigmas"};
  * with DifferentialDiffusion the thresholds are (t(sigma) - t(sigma_min)) / (t(sigmas[0]) - t(sigma_min));
  * NO BEHAVIOUR CHANGE: with the option off (a mask present or not), and with the option on and no mask, every sampler's trajectory is the
    bits of a run that knows of no mask; with the option on and m == 1 as well;
  * with a mask that is 0 on the left half the kept half ends at latent_image (this fails where the keyword is swallowed)."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_preview_cpu import _ToyInner, _ToyPatcher, host_update_arithmetic      # noqa: E402,F401  (the fixture is used by name)
from lightdiffusion_amd import detailer as D                                     # noqa: E402
from lightdiffusion_amd import nodes as N                                        # noqa: E402
from lightdiffusion_amd import ops                                               # noqa: E402
from lightdiffusion_amd import sampling as S                                     # noqa: E402

SAMPLERS = [("euler_ancestral", {}), ("dpmpp_2m_sde", {}), ("dpm_adaptive", {})]
STEPS = 4


def cond(seed):
    return [[torch.randn(1, 77, 8, generator=torch.Generator().manual_seed(seed)), {}]]


def latent_of(b=2, mask=None, zero=False):
    g = torch.Generator().manual_seed(7)
    lat = {"samples": torch.zeros(b, 4, 3, 5) if zero else torch.randn(b, 4, 3, 5, generator=g)}
    if mask is not None:
        lat["noise_mask"] = mask
    return lat


class CountingInner(_ToyInner):
    def __init__(self):
        self.calls = 0

    def apply_model(self, x, t, c_crossattn=None, **kw):
        self.calls += 1
        return super().apply_model(x, t, c_crossattn=c_crossattn, **kw)


def patcher():
    p = _ToyPatcher()
    p.model = CountingInner()
    return p


def run(sampler, lat, model=None, **kw):
    """-> (final samples, [x after every step]) of one common_ksampler run"""
    seen = []
    model = patcher() if model is None else model
    out = S.common_ksampler(model, 5, STEPS, 3.0, sampler, "normal", cond(1), cond(2), lat, callback=lambda d: seen.append(d["x"].clone()), **kw)
    return out[0]["samples"], seen


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def left_half_mask(h=3, w=5):
    m = torch.ones(h, w)
    m[:, : w // 2] = 0.0
    return m


# ------------------------------------------------------------------ prepare_mask
def test_prepare_mask_is_the_interpolate_restatement():
    g = torch.Generator().manual_seed(3)
    shape = (2, 4, 3, 5)
    for mask in (torch.rand(24, 40, generator=g), torch.rand(1, 24, 40, generator=g), torch.rand(2, 1, 24, 40, generator=g), torch.rand(3, 5, generator=g),
                 torch.rand(3, 1, 6, 10, generator=g)):
        got = S.prepare_mask(mask, shape, torch.device("cpu"))
        want = F.interpolate(mask.reshape(-1, 1, mask.shape[-2], mask.shape[-1]), size=(3, 5), mode="bilinear")
        want = want[:2] if want.shape[0] > 2 else want.repeat(2 // want.shape[0], 1, 1, 1)
        assert tuple(got.shape) == (2, 1, 3, 5) and got.dtype == torch.float32 and got.is_contiguous()
        assert same_bits(got, want)
    assert same_bits(S.prepare_mask(torch.rand(3, 5, generator=torch.Generator().manual_seed(1)), shape, "cpu")[0],
                     torch.rand(3, 5, generator=torch.Generator().manual_seed(1))[None]), "a mask on the latent grid is taken as it is"
    # upstream's repeat: 2 -> 5 is the pair repeated and cut
    five = S.repeat_to_batch_size(torch.arange(2.0).view(2, 1), 5)
    assert five.flatten().tolist() == [0.0, 1.0, 0.0, 1.0, 0.0]


def test_set_latent_noise_mask_copies_the_dict():
    lat = latent_of()
    m = torch.rand(24, 40)
    (out,) = N.SetLatentNoiseMask().set_mask(lat, m)
    assert "noise_mask" not in lat and out["samples"] is lat["samples"]
    assert tuple(out["noise_mask"].shape) == (1, 1, 24, 40) and torch.equal(out["noise_mask"][0, 0], m)
    assert tuple(N.SetLatentNoiseMask().set_mask(lat, torch.rand(2, 24, 40))[0]["noise_mask"].shape) == (2, 1, 24, 40)


# ------------------------------------------------------------------ the host path of the two blends, and the checks in front of them
def test_blend_host_path_is_the_expression_and_refuses_bad_shapes():
    g = torch.Generator().manual_seed(11)
    x, lat, noise = (torch.randn(3, 4, 5, 7, generator=g) for _ in range(3))
    sigma = torch.tensor([0.3, 2.5, 14.0])
    for mshape in ((1, 1, 5, 7), (3, 1, 5, 7), (3, 4, 5, 7), (1, 4, 5, 7)):
        m = torch.rand(mshape, generator=g)
        want = x * m + (noise * sigma.view(3, 1, 1, 1) + lat) * (1.0 - m)
        assert same_bits(ops.inpaint_in(x, m, lat, noise, sigma), want)
        xx = x.clone()
        assert ops.inpaint_in(xx, m, lat, noise, sigma, out=xx) is xx and same_bits(xx, want)
        den = x.clone()
        assert ops.inpaint_out_(den, m, lat) is den and same_bits(den, x * m + lat * (1.0 - m))
    m = torch.rand(1, 1, 5, 7, generator=g)
    with pytest.raises(ValueError, match="mask of shape"):
        ops.inpaint_in(x, torch.rand(2, 1, 5, 7), lat, noise, sigma)
    with pytest.raises(ValueError, match="mask of shape"):
        ops.inpaint_out_(x.clone(), torch.rand(1, 2, 5, 7), lat)
    with pytest.raises(ValueError, match="mask of shape"):
        ops.inpaint_out_(x.clone(), torch.rand(1, 1, 5, 6), lat)
    with pytest.raises(ValueError, match="noise of shape"):
        ops.inpaint_in(x, m, lat, noise[:2], sigma)
    with pytest.raises(ValueError, match="sigma"):
        ops.inpaint_in(x, m, lat, noise, sigma[:2])
    with pytest.raises(ValueError, match="sigma"):
        ops.inpaint_in(x, m, lat, noise, 0.5)
    with pytest.raises(ValueError, match="dtype"):
        ops.inpaint_in(x, m.double(), lat, noise, sigma)
    with pytest.raises(ValueError, match="contiguous"):
        ops.inpaint_out_(x.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2), m, lat)
    with pytest.raises(ValueError, match="latent"):
        ops.inpaint_out_(x[0], m, lat)


# ------------------------------------------------------------------ the wrapper and the mask function
@pytest.mark.parametrize("sampler,extra", SAMPLERS)
def test_mask_function_is_asked_once_per_model_call(host_update_arithmetic, sampler, extra):
    model = patcher()
    asked = []

    def fn(sigma, mask, extra_options):
        asked.append((sigma.clone(), mask, dict(extra_options, inner=extra_options["model"].inner_model)))      # (the guider drops it after the run)
        return mask
    model.model_options["denoise_mask_function"] = fn
    pixel_mask = torch.rand(24, 40, generator=torch.Generator().manual_seed(2))
    run(sampler, latent_of(mask=pixel_mask), model, apply_noise_mask=True)
    assert model.model.calls == len(asked) >= STEPS
    sigmas = S.calculate_sigmas(model.model.model_sampling, "normal", STEPS)
    prepared = S.prepare_mask(pixel_mask, (2, 4, 3, 5), "cpu")
    for sigma, mask, eo in asked:
        assert tuple(sigma.shape) == (2,) and sigma.dtype == torch.float32 and float(sigma[0]) == float(sigma[1])
        assert same_bits(mask, prepared), "the mask function is handed the run's prepared mask, not an earlier answer"
        assert set(eo) == {"model", "sigmas", "inner"} and torch.equal(eo["sigmas"], sigmas)
        assert eo["inner"] is model.model and isinstance(eo["model"], S.CFGGuider)
    if sampler != "dpm_adaptive":
        assert [float(s[0]) for s, _, _ in asked] == [float(s) for s in sigmas[:-1]]
    # without the option the function is never asked
    asked.clear()
    run(sampler, latent_of(mask=pixel_mask), model)
    assert not asked


@pytest.mark.parametrize("sampler,extra", SAMPLERS)
def test_differential_diffusion_thresholds(host_update_arithmetic, sampler, extra):
    base = patcher()
    ms = base.model.model_sampling
    dd = D.DifferentialDiffusion()
    seen = []

    def fn(sigma, mask, extra_options):
        out = dd.forward(sigma, mask, extra_options)
        seen.append((float(sigma[0]), mask, out))
        return out
    base.model_options["denoise_mask_function"] = fn
    ramp = torch.linspace(0.0, 1.0, 15).view(1, 1, 3, 5).contiguous()               # every threshold cuts it somewhere else
    run(sampler, latent_of(mask=ramp), base, apply_noise_mask=True)
    sigmas = S.calculate_sigmas(ms, "normal", STEPS)
    t = lambda s: int(ms.timestep(torch.as_tensor(s)))
    assert len(seen) == base.model.calls >= STEPS
    thresholds = set()
    for sigma, mask, out in seen:
        thr = (t(sigma) - t(ms.sigma_min)) / (t(sigmas[0]) - t(ms.sigma_min))
        thresholds.add(thr)
        assert torch.equal(out, (mask >= torch.tensor(thr, dtype=torch.float32)).to(torch.float32)), (sigma, thr)
        assert set(out.unique().tolist()) <= {0.0, 1.0}
    assert max(thresholds) == 1.0 and len(thresholds) >= 3, "the first call is at sigmas[0]; later ones open the mask up"


# ------------------------------------------------------------------ no behaviour change
@pytest.mark.parametrize("sampler,extra", SAMPLERS)
def test_option_off_and_option_on_without_a_mask_change_no_bit(host_update_arithmetic, sampler, extra):
    out0, traj0 = run(sampler, latent_of())
    assert len(traj0) >= STEPS
    mask = left_half_mask()
    cases = {
        "a mask, no option": run(sampler, latent_of(mask=mask)),
        "a mask, the option off": run(sampler, latent_of(mask=mask), apply_noise_mask=False),
        "the option on, no mask": run(sampler, latent_of(), apply_noise_mask=True),
    }
    for name, (out, traj) in cases.items():
        assert same_bits(out, out0), name
        assert len(traj) == len(traj0) and all(same_bits(a, b) for a, b in zip(traj, traj0)), name
    # ... and a mask function on the model is not asked on those routes
    model = patcher()
    model.model_options["denoise_mask_function"] = lambda *a, **k: pytest.fail("asked")
    assert same_bits(run(sampler, latent_of(mask=mask), model)[0], out0)
    assert same_bits(run(sampler, latent_of(), model, apply_noise_mask=True)[0], out0)


@pytest.mark.parametrize("sampler,extra", SAMPLERS)
@pytest.mark.parametrize("zero", [False, True])
def test_a_mask_of_ones_changes_no_bit(host_update_arithmetic, sampler, extra, zero):
    out0, traj0 = run(sampler, latent_of(zero=zero))
    for ones in (torch.ones(3, 5), torch.ones(2, 1, 24, 40)):
        out, traj = run(sampler, latent_of(mask=ones, zero=zero), apply_noise_mask=True)
        assert same_bits(out, out0)
        assert len(traj) == len(traj0) and all(same_bits(a, b) for a, b in zip(traj, traj0))


# ------------------------------------------------------------------ the feature
@pytest.mark.parametrize("sampler,extra", SAMPLERS)
def test_kept_half_returns_to_the_latent(host_update_arithmetic, sampler, extra):
    """m = 0 on the left half.  euler_ancestral's last step (to sigma = 0) is x <- 0 x + 1 denoised and dpmpp_2m_sde's is x = denoised, and the
    blend leaves denoised = 0 den + 1 latent there: the kept half IS latent_image.  dpm_adaptive stops at sigma_end = sigmas[-2] > 0: there eps =
    (x - latent) / sigma is one constant e at every evaluation — e = (x0 - latent) / sigmas[0], the run's noise (times sqrt(1 + sigma^2) / sigma
    where KSAMPLER starts from max_denoise) — which the solver integrates exactly, so the kept half ends at latent + sigma_end e.  Compared here
    to 1e-4 of sigma_end |e| (the solver stops within 1e-5 of t_end; the GPU test derives the rounding bound): it is nowhere near a redraw."""
    lat = latent_of(mask=left_half_mask())
    L = lat["samples"]
    out, _ = run(sampler, lat, apply_noise_mask=True)
    free, _ = run(sampler, latent_of())
    kept, redrawn = (slice(None), slice(None), slice(None), slice(0, 2)), (slice(None), slice(None), slice(None), slice(2, 5))
    if sampler == "dpm_adaptive":
        ms = _ToyInner.model_sampling
        sigmas = S.calculate_sigmas(ms, "normal", STEPS)
        x0 = ms.noise_scaling(sigmas[0], S.prepare_noise(L, 5), L, max_denoise=True)        # 4 steps of the whole schedule start at sigma_max
        e = (x0.double() - L.double()) / float(sigmas[0])
        want = L.double() + float(sigmas[-2]) * e
        assert (out[kept].double() - want[kept]).abs().max() <= 1e-4 * float(sigmas[-2]) * e[kept].abs().max()
    else:
        assert torch.equal(out[kept], L[kept])
    assert not torch.allclose(out[redrawn], L[redrawn], atol=1e-2), "the other half is drawn"
    assert not torch.allclose(free[kept], L[kept], atol=1e-2), "and without the option the kept half is drawn too"
