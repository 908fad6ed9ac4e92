"""Host mirror of the reference's sampling call surface (LD.py:827-1351, 2435-3203, 6657-6725), driving the
MI355X UNet.  Same names, argument meaning and error behaviour; the arithmetic on latents runs on the device
through the C ABI (cfg mix, sampler axpy), the schedule math stays on the host in fp32 exactly as the reference
computes it.

RNG parity: the initial noise comes from `torch.manual_seed(seed)` on the CPU generator
(prepare_noise, LD.py:3145-3153).  Euler-ancestral's per-step noise is `torch.randn_like(x)` on x's device in the
reference — on its CPU path that is the *global CPU generator*, so this mirror draws it on the host in the same order
and uploads it; for a sharded batch every rank draws the full-batch tensor and slices its rows.
"""
from __future__ import annotations

import itertools
import math
from typing import Callable, List, Optional

import torch

from . import ops

_CTX_TOKENS = itertools.count(1)   # per-run context tokens (never reused within a process)

LATENT_SCALE = 0.18215          # SD15.scale_factor, LD.py:137-147
KSAMPLER_NAMES = ["euler_ancestral", "dpm_adaptive", "dpmpp_2m_sde"]          # LD.py:2725-2729
SCHEDULER_NAMES = ["normal", "karras", "exponential", "sgm_uniform", "simple", "ddim_uniform"]   # LD.py:3034-3041


# ------------------------------------------------------------------ model sampling (EPS + ModelSamplingDiscrete)
class ModelSampling:
    """LD.py:1258-1351.  1000-entry sigma table from scaled-linear betas (0.00085 → 0.012), built in fp64."""

    sigma_data = 1.0

    def __init__(self, linear_start: float = 0.00085, linear_end: float = 0.012, timesteps: int = 1000):
        betas = torch.linspace(linear_start ** 0.5, linear_end ** 0.5, timesteps, dtype=torch.float64) ** 2
        acp = torch.cumprod(1.0 - betas, dim=0)
        sig = ((1 - acp) / acp) ** 0.5
        self.sigmas = sig.float()
        self.log_sigmas = sig.log().float()
        self.num_timesteps = timesteps

    @property
    def sigma_min(self):
        return self.sigmas[0]

    @property
    def sigma_max(self):
        return self.sigmas[-1]

    def timestep(self, sigma: torch.Tensor) -> torch.Tensor:
        d = sigma.detach().float().cpu().log() - self.log_sigmas[:, None]
        return d.abs().argmin(dim=0).view(sigma.shape)

    def timestep_on_device(self, sigma: torch.Tensor) -> torch.Tensor:
        """`timestep` for a sigma that lives on a device, without reading it on the host: the same log, difference and argmin as torch
        operations on sigma's device (the table is uploaded once per device).  The host and the device round fp32 log alike up to its last bit,
        so the index differs from `timestep`'s only for a sigma within that of the midpoint between two table entries."""
        cache = self.__dict__.setdefault("_log_sigmas_on", {})
        table = cache.get(sigma.device)
        if table is None:
            table = cache[sigma.device] = self.log_sigmas.to(sigma.device)
        d = sigma.detach().float().log() - table[:, None]
        return d.abs().argmin(dim=0).view(sigma.shape)

    def sigma(self, timestep: torch.Tensor) -> torch.Tensor:
        t = torch.clamp(timestep.float().cpu(), min=0, max=len(self.sigmas) - 1)
        lo, hi, w = t.floor().long(), t.ceil().long(), t.frac()
        return ((1 - w) * self.log_sigmas[lo] + w * self.log_sigmas[hi]).exp()

    def percent_to_sigma(self, percent: float) -> float:
        """Upstream's ModelSamplingDiscrete.percent_to_sigma (the reference has none): the sigma at a fraction of the run, for the
        start_percent / end_percent of a conditioning entry — beyond every sigma at 0 and before, 0 at 1 and after."""
        if percent <= 0.0:
            return 999999999.9
        if percent >= 1.0:
            return 0.0
        return float(self.sigma(torch.tensor((1.0 - percent) * 999.0)))

    # EPS
    def noise_scaling(self, sigma, noise, latent_image, max_denoise=False):
        scale = math.sqrt(1.0 + float(sigma) ** 2.0) if max_denoise else float(sigma)
        return noise * scale + latent_image

    def inverse_noise_scaling(self, sigma, latent):
        return latent


def get_sigmas_karras(n, sigma_min, sigma_max, rho=7.0, device="cpu"):
    """LD.py:831-837."""
    ramp = torch.linspace(0, 1, n)
    lo, hi = sigma_min ** (1 / rho), sigma_max ** (1 / rho)
    sig = (hi + ramp * (lo - hi)) ** rho
    return torch.cat([sig, sig.new_zeros([1])]).to(device)


def normal_scheduler(model_sampling: ModelSampling, steps: int) -> torch.Tensor:
    """LD.py:2639-2651: linspace in t, log-sigma interpolation."""
    s = model_sampling
    ts = torch.linspace(s.timestep(s.sigma_max), s.timestep(s.sigma_min), steps)
    return torch.FloatTensor([float(s.sigma(t)) for t in ts] + [0.0])


def calculate_sigmas(model_sampling: ModelSampling, scheduler_name: str, steps: int) -> torch.Tensor:
    """LD.py:3045-3054: only `karras` and `normal` exist in the reference."""
    if scheduler_name == "karras":
        return get_sigmas_karras(steps, float(model_sampling.sigma_min), float(model_sampling.sigma_max))
    if scheduler_name == "normal":
        return normal_scheduler(model_sampling, steps)
    raise ValueError(f"unknown scheduler '{scheduler_name}' (the reference implements 'karras' and 'normal')")


def get_ancestral_step(sigma_from, sigma_to, eta=1.0):
    """LD.py:844-850."""
    sigma_up = min(sigma_to, eta * (sigma_to ** 2 * (sigma_from ** 2 - sigma_to ** 2) / sigma_from ** 2) ** 0.5)
    return (sigma_to ** 2 - sigma_up ** 2) ** 0.5, sigma_up


def prepare_noise(latent_image: torch.Tensor, seed: int, noise_inds=None) -> torch.Tensor:
    """LD.py:3145-3153: CPU generator seeded by `seed`, fp32."""
    gen = torch.manual_seed(seed)
    return torch.randn(latent_image.size(), dtype=latent_image.dtype, layout=latent_image.layout, generator=gen, device="cpu")


def host_noise_sampler(x: torch.Tensor, rows: Optional[slice] = None, full_batch: Optional[int] = None) -> Callable:
    """default_noise_sampler (LD.py:853-854) for a device-resident x: draw on the host's global generator, upload.
    `rows`/`full_batch`: draw the whole global batch and keep this rank's rows (batch sharding)."""
    shape = list(x.shape)
    if full_batch is not None:
        shape[0] = full_batch

    def sample(sigma, sigma_next):
        n = torch.randn(shape, dtype=x.dtype)
        if rows is not None:
            n = n[rows]
        return n.to(x.device, non_blocking=True)
    return sample


class IIDIntervalNoise:
    """Stand-in for BrownianTreeNoiseSampler (LD.py:889-903, third-party torchsde, absent): the sampler queries
    consecutive disjoint sigma intervals once each and divides by sqrt(|t1 - t0|), so the draws are iid N(0,1).
    Same distribution, different stream of numbers than torchsde — 'parity unpinned' for eta > 0 with default noise."""

    def __init__(self, x: torch.Tensor, seed: Optional[int]):
        self.gen = torch.Generator().manual_seed(0 if seed is None else int(seed) & 0x7FFFFFFFFFFFFFFF)
        self.shape, self.dtype, self.device = x.shape, x.dtype, x.device

    def __call__(self, sigma, sigma_next):
        return torch.randn(self.shape, dtype=self.dtype, generator=self.gen).to(self.device, non_blocking=True)


# ------------------------------------------------------------------ k-diffusion samplers on device latents
def _interrupted(extra_args) -> bool:
    stop = (extra_args or {}).get("should_stop")      # replaces the reference's global app.interrupt_flag (LD.py:922)
    return bool(stop and stop())


@torch.no_grad()
def sample_euler_ancestral(model, x, sigmas, extra_args=None, callback=None, disable=None, eta=1.0, s_noise=1.0, noise_sampler=None):
    """LD.py:907-941.  x fp32 on the device; one fused axpy per step: x <- x + d*dt + noise*s_noise*sigma_up."""
    extra_args = {} if extra_args is None else extra_args
    noise_sampler = host_noise_sampler(x) if noise_sampler is None else noise_sampler
    s_in = x.new_ones([x.shape[0]])
    sig = [float(s) for s in sigmas]
    x = x.clone()
    for i in range(len(sig) - 1):
        if _interrupted(extra_args):
            break
        denoised = model(x, sig[i] * s_in, **extra_args)
        sigma_down, sigma_up = get_ancestral_step(sig[i], sig[i + 1], eta=eta)
        r = (sigma_down - sig[i]) / sig[i]                       # d*dt = (x - denoised) * r
        if sig[i + 1] > 0:
            ops.axpby_(x, 1.0 + r, denoised, -r, noise_sampler(sig[i], sig[i + 1]), s_noise * sigma_up)
        else:
            ops.axpby_(x, 1.0 + r, denoised, -r)
        if callback is not None:
            callback({"x": x, "i": i, "sigma": sig[i], "denoised": denoised})
    return x


@torch.no_grad()
def sample_dpmpp_2m_sde(model, x, sigmas, extra_args=None, callback=None, disable=None, eta=1.0, s_noise=1.0, noise_sampler=None,
                        solver_type="midpoint"):
    """LD.py:1174-1244.  eta = 0 is deterministic DPM-Solver++(2M) ("DPM++ 2M" of the configs)."""
    extra_args = {} if extra_args is None else extra_args
    if solver_type not in ("midpoint", "heun"):
        raise ValueError("solver_type must be 'midpoint' or 'heun'")
    if noise_sampler is None and eta:
        noise_sampler = IIDIntervalNoise(x, extra_args.get("seed"))
    s_in = x.new_ones([x.shape[0]])
    sig = torch.as_tensor(sigmas, dtype=torch.float32).cpu()
    x = x.clone()
    old_denoised, h_last, h = None, None, None
    for i in range(len(sig) - 1):
        if _interrupted(extra_args):
            break
        denoised = model(x, float(sig[i]) * s_in, **extra_args)
        if sig[i + 1] == 0:
            x = denoised.clone()
        else:
            t, s = -sig[i].log(), -sig[i + 1].log()
            h = s - t
            eta_h = eta * h
            a = float(sig[i + 1] / sig[i] * (-eta_h).exp())
            c1 = float((-h - eta_h).expm1().neg())
            if old_denoised is None:
                ops.axpby_(x, a, denoised, c1)
            else:
                r = h_last / h
                k = float(((-h - eta_h).expm1().neg() / (-h - eta_h) + 1) * (1 / r)) if solver_type == "heun" \
                    else float(0.5 * (-h - eta_h).expm1().neg() * (1 / r))
                ops.axpby_(x, a, denoised, c1 + k, old_denoised, -k)
            if eta:
                amp = float(sig[i + 1] * (-2 * eta_h).expm1().neg().sqrt() * s_noise)
                ops.axpby_(x, 1.0, noise_sampler(float(sig[i]), float(sig[i + 1])), amp)
        if callback is not None:
            callback({"x": x, "i": i, "sigma": float(sig[i]), "denoised": denoised})
        old_denoised, h_last = denoised, h
    return x


class _PIDStep:
    """PID step-size controller of DPM-Solver-12/23 (LD.py:944-973): h <- h * limiter(prod inv_err_k ** b_k)."""

    def __init__(self, h, pcoeff, icoeff, dcoeff, order, accept_safety, eps=1e-8):
        self.h, self.accept_safety, self.eps = h, accept_safety, eps
        self.b = ((pcoeff + icoeff + dcoeff) / order, -(pcoeff + 2 * dcoeff) / order, dcoeff / order)
        self.hist = None

    def propose(self, error: float) -> bool:
        inv = 1.0 / (float(error) + self.eps)
        if self.hist is None:
            self.hist = [inv, inv, inv]
        self.hist[0] = inv
        factor = self.hist[0] ** self.b[0] * self.hist[1] ** self.b[1] * self.hist[2] ** self.b[2]
        factor = 1 + math.atan(factor - 1)
        accept = factor >= self.accept_safety
        if accept:
            self.hist[2], self.hist[1] = self.hist[1], self.hist[0]
        self.h = self.h * factor
        return accept


@torch.no_grad()
def sample_dpm_adaptive(model, x, sigma_min, sigma_max, extra_args=None, callback=None, disable=None, order=3, rtol=0.05, atol=0.0078,
                        h_init=0.05, pcoeff=0.0, icoeff=1.0, dcoeff=0.0, accept_safety=0.81, eta=0.0, s_noise=1.0,
                        noise_sampler=None, return_info=False):
    """DPM-Solver-12/23 with adaptive steps (LD.py:976-1170) — the reference GUI's default sampler (LD.py:10572-10576).
    Three UNet evaluations per proposed step (eps at s, at s + h/3, at s + 2h/3; the 2nd-order estimate shares the first
    two), embedded error estimate, PID step control in t = -log(sigma).  The reference's variant adds no noise (su = 0)."""
    if sigma_min <= 0 or sigma_max <= 0:
        raise ValueError("sigma_min and sigma_max must not be 0")
    extra_args = {} if extra_args is None else extra_args
    sig = lambda t: (-t).exp()                                       # t is a 0-dim fp32 tensor, like the reference's
    ones = x.new_ones([x.shape[0]])

    def eps_at(xx, t):
        s = sig(t)
        return (xx - model(xx, float(s) * ones, **extra_args)) / float(s)

    t_start, t_end = -torch.tensor(float(sigma_max)).log(), -torch.tensor(float(sigma_min)).log()
    forward = bool(t_end > t_start)
    pid = _PIDStep(abs(h_init) * (1 if forward else -1), pcoeff, icoeff, dcoeff, 1.5 if eta else order, accept_safety)
    atol_t, rtol_t = torch.tensor(atol, device=x.device), torch.tensor(rtol, device=x.device)
    s, x_prev = t_start, x
    info = {"steps": 0, "nfe": 0, "n_accept": 0, "n_reject": 0}
    r1, r2 = 1.0 / 3.0, 2.0 / 3.0
    while (s < t_end - 1e-5) if forward else (s > t_end + 1e-5):
        if _interrupted(extra_args):
            break
        t = torch.minimum(t_end, s + pid.h) if forward else torch.maximum(t_end, s + pid.h)
        h = t - s
        e0 = eps_at(x, s)
        s1, s2 = s + r1 * h, s + r2 * h
        u1 = x - float(sig(s1) * (r1 * h).expm1()) * e0
        e1 = eps_at(u1, s1)
        x_low = x - float(sig(t) * h.expm1()) * e0 - float(sig(t) / (2 * r1) * h.expm1()) * (e1 - e0)
        u2 = x - float(sig(s2) * (r2 * h).expm1()) * e0 - float(sig(s2) * (r2 / r1) * ((r2 * h).expm1() / (r2 * h) - 1)) * (e1 - e0)
        e2 = eps_at(u2, s2)
        x_high = x - float(sig(t) * h.expm1()) * e0 - float(sig(t) / r2 * (h.expm1() / h - 1)) * (e2 - e0)
        delta = torch.maximum(atol_t, rtol_t * torch.maximum(x_low.abs(), x_prev.abs()))
        error = float(torch.linalg.norm((x_low - x_high) / delta) / x.numel() ** 0.5)
        if pid.propose(error):
            x_prev, x, s = x_low, x_high, t
            info["n_accept"] += 1
        else:
            info["n_reject"] += 1
        info["nfe"] += order
        info["steps"] += 1
        if callback is not None:
            callback({"x": x, "i": info["steps"], "sigma": float(sig(s)), "denoised": None})
    return (x, info) if return_info else x


# ------------------------------------------------------------------ guidance
def convert_cond(cond):
    """LD.py:2287-2297 (cond = [[tensor, {..}], ...])."""
    out = []
    for c in cond:
        d = c[1].copy()
        d["cross_attn"] = c[0]
        out.append(d)
    return out


def _cat_ctx(ctx_list: List[torch.Tensor]) -> torch.Tensor:
    """CONDCrossAttn.concat (LD.py:647-663): pad shorter contexts by repetition up to the lcm of the token counts."""
    tgt = 1
    for c in ctx_list:
        tgt = abs(tgt * c.shape[1]) // math.gcd(tgt, c.shape[1])
    return torch.cat([c if c.shape[1] == tgt else c.repeat(1, tgt // c.shape[1], 1) for c in ctx_list])


def _ctx_rows(c: dict, b: int) -> torch.Tensor:
    """an entry's context for a latent batch of b: its own rows, or its one row b times"""
    t = c["cross_attn"]
    if t.shape[0] != b:
        if t.shape[0] != 1:
            raise RuntimeError(f"conditioning batch {t.shape[0]} does not match latent batch {b}")
        t = t.expand(b, -1, -1)
    return t


# ------------------------------------------------------------------ regional conditioning (model_options["ld_cond_areas"])
REGIONAL_MAX_ENTRIES = ops.REGIONAL_MAX_ENTRIES     # entries active in one step: the combine kernel's table travels in its arguments
_NO_START, _NO_END = float("inf"), float("-inf")


def _fp32(v: float) -> float:
    return float(torch.tensor(float(v), dtype=torch.float32))


def _cond_is_keyed(c: dict) -> bool:
    """does the entry ask for anything but the whole latent at weight 1?  (strength 1 counts as none; a step range does not matter to an
    entry that is active)"""
    return c.get("area") is not None or c.get("mask") is not None or c.get("strength", 1.0) != 1.0


def _host_sigma(timestep: torch.Tensor) -> float:
    """THE host read of a regional step: sigma[0], which upstream compares with an entry's timestep range on the host (get_area_and_mult).
    Called once per step, and only in a run in which some entry carries a range; a skipped entry then costs no UNet work."""
    return float(timestep[0])


def resolve_areas_and_cond_masks(conds: List[dict], b: int, h: int, w: int, device) -> List[dict]:
    """Upstream's resolve_areas_and_cond_masks (the reference's, LD.py:2654-2667, has an empty body), on copies: percentage areas become
    latent units, a mask becomes a contiguous fp32 [Bm, h, w] on `device` with Bm in {1, b} (bilinear resize, align_corners=False, where it has
    another size), and with set_area_to_bounds the area becomes the bounding box of max_b |mask| > 0, its sides raised to at least 8 and cut
    at the latent's edge ((8, 8, 0, 0) for a mask of zeros)."""
    out = []
    for c in conds:
        c = c.copy()
        area = c.get("area")
        if area is not None:
            if len(area) == 5 and area[0] == "percentage":
                area = (max(1, round(area[1] * h)), max(1, round(area[2] * w)), round(area[3] * h), round(area[4] * w))
            if len(area) != 4:
                raise ValueError(f"a conditioning area is (h, w, y, x) or ('percentage', h, w, y, x), got {tuple(area)!r}")
            c["area"] = tuple(int(v) for v in area)
        if c.get("mask") is not None:
            mask = c["mask"].to(device=device, dtype=torch.float32)
            if mask.dim() == 2:
                mask = mask.unsqueeze(0)
            if mask.dim() != 3:
                raise ValueError(f"a conditioning mask is [Bm, Hm, Wm] or [Hm, Wm], got {tuple(mask.shape)}")
            if tuple(mask.shape[1:]) != (h, w):
                mask = torch.nn.functional.interpolate(mask.unsqueeze(1), size=(h, w), mode="bilinear", align_corners=False).squeeze(1)
            if mask.shape[0] not in (1, b):
                mask = repeat_to_batch_size(mask, b)
            mask = mask.contiguous()
            if c.get("set_area_to_bounds", False):
                lit = mask.abs().amax(dim=0) > 0
                ys, xs = torch.nonzero(lit.any(dim=1)).flatten().tolist(), torch.nonzero(lit.any(dim=0)).flatten().tolist()
                if not ys:
                    c["area"] = (8, 8, 0, 0)
                else:
                    y0, x0 = ys[0], xs[0]
                    c["area"] = (min(max(8, ys[-1] - y0 + 1), h - y0), min(max(8, xs[-1] - x0 + 1), w - x0), y0, x0)
            c["mask"] = mask
        out.append(c)
    return out


def calculate_start_end_timesteps(model_sampling: ModelSampling, conds: List[dict]) -> None:
    """Upstream's (LD.py:2654-2667: an empty body): start_percent / end_percent -> timestep_start / timestep_end, as sigmas.  In place: the dicts
    are process_conds' copies."""
    for c in conds:
        if "start_percent" in c:
            c["timestep_start"] = model_sampling.percent_to_sigma(c["start_percent"])
        if "end_percent" in c:
            c["timestep_end"] = model_sampling.percent_to_sigma(c["end_percent"])


def create_cond_with_same_area_if_none(conds: List[dict], c: dict) -> None:
    """Upstream's rule (LD.py:2654-2667: an empty body): an entry `c` with an area needs an entry of the same area in the OTHER list `conds`.
    Candidates are its entries whose area contains c's (one without an area contains everything and loses to any that has one); the one with the
    smallest h * w wins, the earlier one on a tie; unless it has exactly c's area, a copy of it with c's area is appended."""
    if c.get("area") is None:
        return
    ca = c["area"]
    smallest = None
    for x in conds:
        a = x.get("area")
        if a is not None:
            if ca[2] >= a[2] and ca[3] >= a[3] and a[0] + a[2] >= ca[0] + ca[2] and a[1] + a[3] >= ca[1] + ca[3]:
                if smallest is None or smallest.get("area") is None or smallest["area"][0] * smallest["area"][1] > a[0] * a[1]:
                    smallest = x
        elif smallest is None:
            smallest = x
    if smallest is None or smallest.get("area") == ca:
        return
    out = smallest.copy()
    out["area"] = ca
    conds.append(out)


def _max_active(conds: List[dict]) -> int:
    """the largest number of entries one step can have active: ranges are closed sigma intervals, so the maximum is met at an interval's end"""
    spans = [(_fp32(c.get("timestep_end", _NO_END)), _fp32(c.get("timestep_start", _NO_START))) for c in conds]
    return max((sum(1 for lo, hi in spans if lo <= s <= hi) for s in {v for span in spans for v in span}), default=0)


def process_conds(positive: List[dict], negative: List[dict], shape, device, model_sampling: ModelSampling):
    """Upstream's process_conds for the keys this stack honours, once per run (CFGGuider.sample, when model_options["ld_cond_areas"]) ->
    (positive, negative): new lists of new dicts — the caller's are not modified.  Areas and masks are resolved on the latent of `shape`
    ([B, C, H, W]), percent ranges become sigmas, and every entry with an area gets a partner of that area in the other list (positive ->
    negative first, then negative -> positive).  ValueError, before anything is launched: an area that leaves the latent or has a side < 1;
    an unmasked area narrower than 8 on an axis where it has an edge inside the latent (upstream's feather slices wrap around there, which is
    not reproduced); more than REGIONAL_MAX_ENTRIES entries active in one step."""
    b, _, h, w = shape
    positive = resolve_areas_and_cond_masks(positive, b, h, w, device)
    negative = resolve_areas_and_cond_masks(negative, b, h, w, device)
    calculate_start_end_timesteps(model_sampling, positive)
    calculate_start_end_timesteps(model_sampling, negative)
    for c in list(positive):
        create_cond_with_same_area_if_none(negative, c)
    for c in list(negative):
        create_cond_with_same_area_if_none(positive, c)
    for name, conds in (("positive", positive), ("negative", negative)):
        for i, c in enumerate(conds):
            if c.get("area") is None:
                continue
            ah, aw, y, x = c["area"]
            where = f"{name} conditioning entry {i}: area (h, w, y, x) = {c['area']}"
            if ah < 1 or aw < 1:
                raise ValueError(f"{where} has a side < 1")
            if y < 0 or x < 0 or y + ah > h or x + aw > w:
                raise ValueError(f"{where} leaves the {h} x {w} latent")
            if c.get("mask") is None and ((ah < 8 and (y != 0 or y + ah < h)) or (aw < 8 and (x != 0 or x + aw < w))):
                raise ValueError(f"{where} is narrower than 8 on an axis where it has an edge inside the {h} x {w} latent: the 8-pixel feather "
                                 f"does not fit (upstream's slices wrap around there; that is not reproduced)")
    n = _max_active(positive + negative)
    if n > REGIONAL_MAX_ENTRIES:
        raise ValueError(f"{n} conditioning entries are active in one step; at most {REGIONAL_MAX_ENTRIES} are supported")
    return positive, negative


class _RegionalGroup:
    """the entries of one area shape that are active together: one eager UNet call on k * B rows"""

    def __init__(self, windows, ctx, token, cond_or_uncond):
        self.windows, self.ctx, self.token, self.cond_or_uncond = windows, ctx, token, cond_or_uncond


def _regional_plan(active, b: int, H: int, W: int):
    """What a step does for one set of active entries [(list, entry)...] in the order [cond.., uncond..] (upstream's to-run list, LD.py:2505):
    ("plain", uncond, cond) when the existing route serves it — one unkeyed entry per list — else ("regional", groups, table): the entries
    grouped by area shape in the order a shape first appears, batched in reverse inside a group (LD.py:2507-2516 when everything fits one batch),
    and the combine's table in the order the entries were batched.  Each group's context is concatenated once and tagged with a token of its
    own, so the resident K / V are re-projected only when the group on the device changes."""
    if sum(1 for l, _ in active if l == 0) == 1 and sum(1 for l, _ in active if l == 1) == 1 and not any(_cond_is_keyed(c) for _, c in active):
        return ("plain", [c for l, c in active if l == 1], [c for l, c in active if l == 0])
    if len(active) > REGIONAL_MAX_ENTRIES:
        raise ValueError(f"{len(active)} conditioning entries are active in one step; at most {REGIONAL_MAX_ENTRIES} are supported")
    by_shape = {}
    for l, c in active:
        area = tuple(c["area"]) if c.get("area") is not None else (H, W, 0, 0)
        by_shape.setdefault(area[:2], []).append((l, c, area))
    groups, table = [], []
    for g, members in enumerate(by_shape.values()):
        members = members[::-1]
        ctx = _cat_ctx([_ctx_rows(c, b) for _, c, _ in members]).contiguous()
        groups.append(_RegionalGroup([area for _, _, area in members], ctx, next(_CTX_TOKENS), [l for l, _, _ in members]))
        for slot, (l, c, area) in enumerate(members):
            table.append(ops.RegionalEntry(l, g, slot, area, float(c.get("strength", 1.0)), c.get("mask"), float(c.get("mask_strength", 1.0))))
    return ("regional", groups, table)


def _regional_step(model, x, timestep, uncond, cond, cond_scale, model_options):
    """One guided step with regional conditioning -> the guided result, or (uncond, cond) single unkeyed lists for the existing route.  The
    plans are kept per run (the guider's per-run model_options) and per set of active entries."""
    b, _, H, W = x.shape
    state = model_options.setdefault("_ld_regional", {})
    key = (b, H, W, id(uncond), id(cond))
    if state.get("key") != key:
        state.clear()
        entries = [(0, c) for c in cond] + [(1, c) for c in uncond]
        spans = [(_fp32(c.get("timestep_end", _NO_END)), _fp32(c.get("timestep_start", _NO_START))) for _, c in entries]
        state.update(key=key, entries=entries, spans=spans, plans={},
                     ranged=any("timestep_start" in c or "timestep_end" in c for _, c in entries), keep=(uncond, cond))
    entries = state["entries"]
    if state["ranged"]:
        s = _host_sigma(timestep)                 # upstream: skipped when sigma[0] > timestep_start or sigma[0] < timestep_end (fp32 values)
        active = tuple(i for i, (lo, hi) in enumerate(state["spans"]) if lo <= s <= hi)
    else:
        active = tuple(range(len(entries)))
    plan = state["plans"].get(active)
    if plan is None:
        plan = state["plans"][active] = _regional_plan([entries[i] for i in active], b, H, W)
    if plan[0] == "plain":
        return plan[1], plan[2]
    _, groups, table = plan
    if not table:                                 # no entry is active: both lists give 0 / 1e-37 (upstream)
        return torch.zeros_like(x)
    wrapper = model_options.get("model_function_wrapper")
    x = x.to(torch.float32).contiguous()
    outs = []
    for grp in groups:
        k = len(grp.windows)
        xs = ops.regional_gather(x, grp.windows)
        ss = torch.cat([timestep] * k)
        c = {"c_crossattn": grp.ctx, "transformer_options": {"cond_or_uncond": grp.cond_or_uncond, "sigmas": timestep, "ld_ctx_token": grp.token}}
        if wrapper is not None:
            out = wrapper(model.apply_model, {"input": xs, "timestep": ss, "c": c, "cond_or_uncond": grp.cond_or_uncond})
        else:
            out = model.apply_model(xs, ss, **c)
        outs.append(out.to(torch.float32).contiguous())
    return ops.regional_combine(outs, table, cond_scale, x.shape)


# ------------------------------------------------------------------ ControlNet (model_options["ld_control"])
def _fill_control_to_uncond(positive: List[dict], negative: List[dict]) -> None:
    """Upstream's apply_empty_x_to_equal_area(filter(control_apply_to_uncond, positive), negative, "control", ...) (the reference's call:
    LD.py:2872-2886): unless a negative entry without an area already carries a control, the controls of the positive entries that ask for it go
    to the negative entries without one, round robin.  In place, on process_control's copies."""
    cond_cnets = [c["control"] for c in positive if c.get("control_apply_to_uncond", False) is True and "area" not in c and c.get("control") is not None]
    if any(c.get("control") is not None for c in negative if "area" not in c):
        return
    others = [i for i, c in enumerate(negative) if "area" not in c]
    if not others:
        return
    for ix, cn in enumerate(cond_cnets):
        i = others[ix % len(others)]
        if negative[i].get("control") is not None:
            negative.append(dict(negative[i], control=cn))
        else:
            negative[i] = dict(negative[i], control=cn)


def control_step_active(timestep_range, sigma0: float) -> bool:
    """upstream's ControlBase.get_control: skipped when t[0] > timestep_range[0] or t[0] < timestep_range[1]; both boundary sigmas are inside"""
    return timestep_range is None or not (sigma0 > timestep_range[0] or sigma0 < timestep_range[1])


def process_control(positive: List[dict], negative: List[dict], model, model_options: dict):
    """Once per run with model_options["ld_control"] (CFGGuider.sample) -> (positive, negative, control): copies of the lists with the
    control_apply_to_uncond fill, and the one ControlNet the run applies (None: no entry carries one), after its pre_run.  What this stack does
    not run is refused here, before anything is launched (NotImplementedError): chained ControlNets, a control on only one of the lists or
    different controls on the entries, control beside regional conditioning (ld_cond_areas), a model that is not driven through the captured
    guided step (the bare model_function_wrapper hook seam, ld_eager_unbatched)."""
    positive, negative = [c.copy() for c in positive], [c.copy() for c in negative]
    _fill_control_to_uncond(positive, negative)
    controls = [c.get("control") for c in positive + negative]
    if all(cn is None for cn in controls):
        return positive, negative, None
    cn = next(c for c in controls if c is not None)
    if any(c is not cn for c in controls):
        raise NotImplementedError("apply_control: every entry of both conditioning lists must carry the SAME ControlNet (ControlNetApply sets "
                                  "control_apply_to_uncond; ControlNetApplyAdvanced takes both lists): a control on one list only, or different "
                                  "controls on different entries, is not supported")
    if getattr(cn, "previous_controlnet", None) is not None:
        raise NotImplementedError("apply_control: chained ControlNets (previous_controlnet) are not supported")
    if model_options.get("ld_cond_areas"):
        raise NotImplementedError("apply_control cannot be combined with apply_cond_areas: control on regional conditioning groups is not supported")
    if len(positive) != 1 or len(negative) != 1:
        raise NotImplementedError("apply_control: one positive and one negative conditioning entry are supported")
    wrapper = model_options.get("model_function_wrapper")
    if not hasattr(wrapper, "cfg_denoise") or model_options.get("ld_eager_unbatched", False):
        raise NotImplementedError("apply_control needs the resident UNet's guided step (cfg_denoise): control on the bare model_function_wrapper "
                                  "hook seam, or with ld_eager_unbatched, is not supported")
    # (a patcher's LoRA patches go to the UNet only: the control branch keeps its loaded weights)
    cn.pre_run(model, model.model_sampling.percent_to_sigma)
    return positive, negative, cn


def sampling_function(model, x, timestep, uncond, cond, cond_scale, model_options=None, seed=None):
    """sampling_function / calc_cond_batch / cfg_function (LD.py:2492-2626): ONE batched UNet call in the order
    [uncond, cond] (the reference reverses its to-run list, LD.py:2515), then uncond + (cond - uncond) * scale.

    Several entries in a conditioning list: the reference runs every entry over the WHOLE latent with weight 1 and averages
    them per list — its `get_area_and_mult` (LD.py:2435-2458) hard-codes area = the full latent and strength = 1.0 and never
    looks at "area", "strength", "mask" or timestep-range keys, so by default neither does this mirror (same images as the
    reference; those keys are inert there).  That case takes one eager UNet call on (len(uncond) + len(cond)) * B samples; the
    single-entry case — every call the reference's own pipelines make — replays the captured hipGraph.

    model_options["ld_cond_areas"] (apply_cond_areas=True on the sampler nodes; off by default) gives the keys upstream's meaning
    (`_regional_step`; the entries are those CFGGuider.sample resolved with `process_conds`): per step the active entries — those whose
    timestep range holds sigma[0] — are grouped by area shape, each group is one eager UNet call on its windows of the latent
    (ops.regional_gather), and ops.regional_combine weighs the outputs by strength, mask and the 8-pixel feather of area edges, normalises per
    list and applies the guidance.  A step whose active entries are one per list and carry no key takes the route above unchanged."""
    model_options = model_options or {}
    b = x.shape[0]
    if model_options.get("ld_cond_areas"):
        routed = _regional_step(model, x, timestep, uncond or [], cond or [], cond_scale, model_options)
        if isinstance(routed, torch.Tensor):
            return routed
        uncond, cond = routed
    if not cond or not uncond:
        raise ValueError("sampling_function needs at least one positive and one negative conditioning entry")
    ctx_of = lambda c: _ctx_rows(c, b)

    # the batched context is step-invariant: build it once per run (cache lives in the guider's per-run model_options) and
    # tag it with a token that is never reused, so the UNet wrapper re-projects K / V^T exactly once per run.
    # Batch order = the reference's: its to-run list [cond.., uncond..] is consumed from the back (LD.py:2505-2515).
    n_u, n_c = len(uncond), len(cond)
    cache = model_options.setdefault("_ld_ctx_cache", {})
    key = (b, id(uncond), id(cond))
    if key not in cache:
        cache.clear()
        cache[key] = (_cat_ctx([ctx_of(c) for c in reversed(uncond)] + [ctx_of(c) for c in reversed(cond)]).contiguous(), next(_CTX_TOKENS))
    ctx, token = cache[key]
    wrapper = model_options.get("model_function_wrapper")
    single = n_u == 1 and n_c == 1
    if single and hasattr(wrapper, "cfg_denoise") and not model_options.get("ld_eager_unbatched", False):
        # MI355X fast path: the whole guided step (cat, UNet on 2B samples, CFG mix) is one replayed hipGraph
        control = model_options.get("_ld_control") if model_options.get("ld_control") else None
        if control is not None:
            # ControlNet (process_control resolved it for this run): inside its step range the step is the control branch on the same
            # [uncond, cond] batch and context, the UNet pair forward with its residuals and the mix — one replayed graph of its own; outside,
            # the ordinary step.  Only a run whose range excludes some step reads sigma[0] on the host (upstream compares it there).
            if control.ranged and not control_step_active(control.timestep_range, _host_sigma(timestep)):
                control = None
        if control is not None:
            return wrapper.cfg_denoise(x, timestep, ctx, cond_scale, token=token, use_graph=model_options.get("ld_use_graph", True), control=control)
        return wrapper.cfg_denoise(x, timestep, ctx, cond_scale, token=token, use_graph=model_options.get("ld_use_graph", True))
    chunks = n_u + n_c
    xs = torch.cat([x] * chunks)
    ss = torch.cat([timestep] * chunks)
    cou = [1] * n_u + [0] * n_c
    c = {"c_crossattn": ctx, "transformer_options": {"cond_or_uncond": cou, "sigmas": timestep, "ld_ctx_token": token}}
    if wrapper is not None:
        out = wrapper(model.apply_model, {"input": xs, "timestep": ss, "c": c, "cond_or_uncond": cou})
    else:
        out = model.apply_model(xs, ss, **c)
    if single:
        return ops.cfg_combine(out.contiguous(), cond_scale)
    parts = out.chunk(chunks)                      # out_conds[i] = sum(output * 1) / count  (LD.py:2569-2591)
    uncond_pred = torch.stack(parts[:n_u]).sum(0) / float(n_u)
    cond_pred = torch.stack(parts[n_u:]).sum(0) / float(n_c)
    return uncond_pred + (cond_pred - uncond_pred) * cond_scale


def repeat_to_batch_size(tensor: torch.Tensor, batch_size: int) -> torch.Tensor:
    """Upstream's helper (the reference's, LD.py:397, returns its argument): dim 0 cut to batch_size, or repeated up to it."""
    if tensor.shape[0] > batch_size:
        return tensor[:batch_size]
    if tensor.shape[0] < batch_size:
        return tensor.repeat([math.ceil(batch_size / tensor.shape[0])] + [1] * (tensor.dim() - 1))[:batch_size]
    return tensor


def prepare_mask(noise_mask: torch.Tensor, shape, device) -> torch.Tensor:
    """Upstream's prepare_mask (the reference has none: its sampler drops the mask): a latent's noise_mask, on the pixel grid or the latent
    grid, as the fp32 denoise mask [B, 1, h, w] of a latent of `shape` on `device` — bilinear resize, repeated to the batch.  ONE channel is kept
    where upstream repeats it over the latent's channels: the blend kernels broadcast it (ops.inpaint_in)."""
    m = noise_mask.reshape((-1, 1, noise_mask.shape[-2], noise_mask.shape[-1])).to(torch.float32)
    m = torch.nn.functional.interpolate(m, size=(shape[2], shape[3]), mode="bilinear")
    return repeat_to_batch_size(m, shape[0]).to(device).contiguous()


class KSamplerX0Inpaint:
    """Upstream's KSamplerX0Inpaint, of which the reference keeps the signature and drops the mask (LD.py:2629-2636): the denoiser of a masked
    run.  Where the mask is 0 the model sees the latent noised to the step's sigma instead of the sampler's x, and its answer there is replaced
    by the latent, so the sampler is led back to `latent_image` where the mask is 0 and draws freely where it is 1.  A "denoise_mask_function"
    in model_options (detailer.DifferentialDiffusion.forward) is asked for the step's mask first.  Two launches beside the model call
    (ops.inpaint_in, ops.inpaint_out_), sigma read on the device: no host read, and the guided step stays the replayed graph.
    `noise` is the run's raw noise (before noise_scaling), `latent_image` the latent after process_latent_in, `denoise_mask` what prepare_mask
    made; all fp32 on the latents' device."""

    def __init__(self, model_wrap, sigmas, noise, latent_image, denoise_mask):
        self.inner_model, self.sigmas = model_wrap, sigmas
        self.noise = noise.to(torch.float32).contiguous()
        self.latent_image = latent_image.to(torch.float32).contiguous()
        self.denoise_mask = denoise_mask

    def __call__(self, x, sigma, model_options=None, seed=None, **_unused):
        model_options = {} if model_options is None else model_options
        mask = self.denoise_mask
        if "denoise_mask_function" in model_options:
            mask = model_options["denoise_mask_function"](sigma, mask, extra_options={"model": self.inner_model, "sigmas": self.sigmas})
        x_in = ops.inpaint_in(x, mask, self.latent_image, self.noise, sigma)
        # the model's answer is the sampler's to keep (cfg_denoise hands out a copy of the captured graph's static buffer, the eager routes a
        # new tensor), so the blend writes into it
        out = self.inner_model(x_in, sigma, model_options=model_options, seed=seed)
        return ops.inpaint_out_(out, mask, self.latent_image)


class KSAMPLER:
    """LD.py:2732-2773.  inpaint_options["apply_denoise_mask"]: honour `denoise_mask` (KSamplerX0Inpaint); without it the mask is dropped, as
    the reference drops it."""

    def __init__(self, sampler_function, extra_options=None, inpaint_options=None):
        self.sampler_function = sampler_function
        self.extra_options = extra_options or {}
        self.inpaint_options = inpaint_options or {}

    def max_denoise(self, model_wrap, sigmas):
        max_sigma = float(model_wrap.inner_model.model_sampling.sigma_max)
        sigma = float(sigmas[0])
        return math.isclose(max_sigma, sigma, rel_tol=1e-05) or sigma > max_sigma

    def sample(self, model_wrap, sigmas, extra_args, callback, noise, latent_image=None, denoise_mask=None, disable_pbar=False):
        ms = model_wrap.inner_model.model_sampling
        raw_noise = noise                                          # the masked route noises the latent per step from it (LD.py:2750-2756)
        noise = ms.noise_scaling(sigmas[0], noise, latent_image, self.max_denoise(model_wrap, sigmas))
        if self.inpaint_options.get("apply_denoise_mask") and denoise_mask is not None:
            model_k = KSamplerX0Inpaint(model_wrap, sigmas, raw_noise, latent_image, denoise_mask)
        else:
            model_k = lambda x, sigma, **kw: model_wrap(x, sigma, **{k: v for k, v in kw.items() if k in ("model_options", "seed")})
        samples = self.sampler_function(model_k, noise, sigmas, extra_args=extra_args, callback=callback, disable=disable_pbar,
                                        **self.extra_options)
        return ms.inverse_noise_scaling(sigmas[-1], samples)


def ksampler(sampler_name, extra_options=None, inpaint_options=None):
    """LD.py:2776-2836."""
    extra_options = extra_options or {}
    if sampler_name == "euler_ancestral":
        fn = lambda model, noise, sigmas, extra_args, callback, disable, **o: sample_euler_ancestral(
            model, noise, sigmas, extra_args=extra_args, callback=callback, disable=disable, **o)
    elif sampler_name == "dpmpp_2m_sde":
        fn = lambda model, noise, sigmas, extra_args, callback, disable, **o: sample_dpmpp_2m_sde(
            model, noise, sigmas, extra_args=extra_args, callback=callback, disable=disable, **o)
    elif sampler_name == "dpm_adaptive":
        def fn(model, noise, sigmas, extra_args, callback, disable, **o):     # dpm_adaptive_function, LD.py:2777-2797
            if len(sigmas) <= 1:
                return noise
            sigma_min = sigmas[-1] if sigmas[-1] != 0 else sigmas[-2]
            return sample_dpm_adaptive(model, noise, float(sigma_min), float(sigmas[0]), extra_args=extra_args, callback=callback,
                                       disable=disable, **o)
    else:
        raise ValueError(f"unknown sampler '{sampler_name}'")
    return KSAMPLER(fn, extra_options, inpaint_options)


class CFGGuider:
    """LD.py:2894-3007."""

    def __init__(self, model_patcher):
        self.model_patcher = model_patcher
        self.model_options = model_patcher.model_options
        self.original_conds = {}
        self.cfg = 1.0

    def set_conds(self, positive, negative):
        self.original_conds = {"positive": convert_cond(positive), "negative": convert_cond(negative)}

    def set_cfg(self, cfg):
        self.cfg = cfg

    def __call__(self, x, timestep, model_options=None, seed=None):
        return sampling_function(self.inner_model, x, timestep, self.conds.get("negative"), self.conds.get("positive"), self.cfg,
                                 model_options=model_options or {}, seed=seed)

    def sample(self, noise, latent_image, sampler, sigmas, denoise_mask=None, callback=None, disable_pbar=False, seed=None):
        # load_models_gpu's place (LD.py:2930): clones share one resident UNet, so the patcher's LoRA patches are swapped in here if they are not
        # the ones applied (one uuid comparison otherwise)
        self.inner_model = self.model_patcher.patch_model() if hasattr(self.model_patcher, "patch_model") else self.model_patcher.model
        device = self.model_patcher.load_device
        self.conds = {k: [dict(c, cross_attn=c["cross_attn"].to(device)) for c in v] for k, v in self.original_conds.items()}
        noise, latent_image = noise.to(device), latent_image.to(device)
        if torch.count_nonzero(latent_image) > 0:                 # don't shift the empty latent (LD.py:2938-2941)
            latent_image = self.inner_model.process_latent_in(latent_image)
        if denoise_mask is not None and getattr(sampler, "inpaint_options", {}).get("apply_denoise_mask"):
            denoise_mask = prepare_mask(denoise_mask, noise.shape, device)      # once per run; on the other route the mask is dropped as it is
        self.model_options = dict(self.model_options)
        self.model_options.pop("_ld_ctx_cache", None)
        self.model_options.pop("_ld_regional", None)
        self.model_options.pop("_ld_control", None)
        control = None
        if self.model_options.get("ld_control"):                  # once per run, on copies: the uncond fill, what is refused, pre_run
            self.conds["positive"], self.conds["negative"], control = process_control(self.conds["positive"], self.conds["negative"],
                                                                                     self.inner_model, self.model_options)
            if control is not None:
                self.model_options["_ld_control"] = control
        if self.model_options.get("ld_cond_areas"):               # once per run, on copies: areas, masks, ranges, the same-area partners
            self.conds["positive"], self.conds["negative"] = process_conds(self.conds["positive"], self.conds["negative"], noise.shape, device,
                                                                           self.inner_model.model_sampling)
        extra_args = {"model_options": self.model_options, "seed": seed}
        samples = sampler.sample(self, sigmas, extra_args, callback, noise, latent_image, denoise_mask, disable_pbar)
        out = self.inner_model.process_latent_out(samples.to(torch.float32))
        if control is not None:
            control.cleanup()                                     # cleanup_models' place (LD.py:2300-2340)
        del self.inner_model, self.conds
        return out


def sample(model, noise, positive, negative, cfg, device, sampler, sigmas, model_options=None, latent_image=None, denoise_mask=None,
           callback=None, disable_pbar=False, seed=None, apply_cond_areas: bool = False, apply_control: bool = False):
    """LD.py:3010-3031.  apply_cond_areas: this run honours the conditioning entries' "area", "strength", "mask" and step-range keys
    (model_options["ld_cond_areas"] on the guider's own copy of the options; sampling_function).  apply_control: this run honours their
    "control" key — a controlnet.ControlNet, as ControlNetApply sets it (model_options["ld_control"]; process_control, sampling_function);
    without it the key is inert, as in the reference."""
    g = CFGGuider(model)
    if apply_cond_areas:
        g.model_options = dict(g.model_options, ld_cond_areas=True)
    if apply_control:
        g.model_options = dict(g.model_options, ld_control=True)
    g.set_conds(positive, negative)
    g.set_cfg(cfg)
    return g.sample(noise, latent_image, sampler, sigmas, denoise_mask, callback, disable_pbar, seed)


class KSampler1:
    """LD.py:3062-3142."""
    SCHEDULERS = SCHEDULER_NAMES
    SAMPLERS = KSAMPLER_NAMES

    def __init__(self, model, steps, device, sampler=None, scheduler=None, denoise=None, model_options=None):
        self.model, self.device, self.scheduler, self.sampler = model, device, scheduler, sampler
        self.set_steps(steps, denoise)
        self.denoise = denoise
        self.model_options = model_options or {}

    def calculate_sigmas(self, steps):
        return calculate_sigmas(self.model.get_model_object("model_sampling"), self.scheduler, steps)

    def set_steps(self, steps, denoise=None):
        self.steps = steps
        if denoise is None or denoise > 0.9999:
            self.sigmas = self.calculate_sigmas(steps)
        else:
            self.sigmas = self.calculate_sigmas(int(steps / denoise))[-(steps + 1):]

    def sample(self, noise, positive, negative, cfg, latent_image=None, denoise_mask=None, sigmas=None, callback=None,
               disable_pbar=False, seed=None, apply_noise_mask: bool = False, apply_cond_areas: bool = False, apply_control: bool = False, **_ignored):
        sigmas = self.sigmas if sigmas is None else sigmas
        sampler = ksampler(self.sampler, inpaint_options={"apply_denoise_mask": True}) if apply_noise_mask else ksampler(self.sampler)
        return sample(self.model, noise, positive, negative, cfg, self.device, sampler, sigmas, self.model_options,
                      latent_image=latent_image, denoise_mask=denoise_mask, callback=callback, disable_pbar=disable_pbar, seed=seed,
                      apply_cond_areas=apply_cond_areas, apply_control=apply_control)


def sample1(model, noise, steps, cfg, sampler_name, scheduler, positive, negative, latent_image, denoise=1.0, noise_mask=None,
            sigmas=None, callback=None, disable_pbar=False, seed=None, apply_noise_mask: bool = False, apply_cond_areas: bool = False,
            apply_control: bool = False, **_ignored):
    """LD.py:3156-3203: returns the samples on the intermediate (CPU) device.  apply_noise_mask: `noise_mask` is the sampler's denoise mask —
    redrawn where it is 1, led back to `latent_image` where it is 0 (KSamplerX0Inpaint); by default it is dropped, as the reference drops it.
    apply_cond_areas: the conditioning entries' area, strength, mask and step-range keys are honoured (sampling_function); by default they are
    inert, as in the reference.  apply_control: the entries' "control" key (a ControlNet) is honoured (sampling_function); by default it is
    inert too."""
    ks = KSampler1(model, steps=steps, device=model.load_device, sampler=sampler_name, scheduler=scheduler, denoise=denoise,
                   model_options=model.model_options)
    out = ks.sample(noise, positive, negative, cfg=cfg, latent_image=latent_image, denoise_mask=noise_mask, sigmas=sigmas,
                    callback=callback, disable_pbar=disable_pbar, seed=seed, apply_noise_mask=apply_noise_mask, apply_cond_areas=apply_cond_areas,
                    apply_control=apply_control)
    return out.to("cpu")


def common_ksampler(model, seed, steps, cfg, sampler_name, scheduler, positive, negative, latent, denoise=1.0, callback=None,
                    apply_noise_mask: bool = False, apply_cond_areas: bool = False, apply_control: bool = False, **_ignored):
    """LD.py:6657-6701.  `callback`: the sampler loop's per-step callback ({"x", "i", "sigma", "denoised"}), e.g. a preview.LatentPreviewer.
    apply_noise_mask: latent["noise_mask"], where there is one, is honoured by the sampler (sample1); by default it is not looked at.
    apply_cond_areas: the conditioning entries' area / strength / mask / step-range keys are honoured (sample1); by default they are inert."""
    latent_image = latent["samples"]
    noise = prepare_noise(latent_image, seed, latent.get("batch_index"))
    masked = {"noise_mask": latent.get("noise_mask"), "apply_noise_mask": True} if apply_noise_mask else {}
    if apply_cond_areas:
        masked["apply_cond_areas"] = True
    if apply_control:                                             # the entries' "control" key is honoured (sample1); by default it is inert
        masked["apply_control"] = True
    samples = sample1(model, noise, steps, cfg, sampler_name, scheduler, positive, negative, latent_image, denoise=denoise, callback=callback, seed=seed,
                      **masked)
    out = latent.copy()
    out["samples"] = samples
    return (out,)
