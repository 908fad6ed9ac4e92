"""ControlNet on the device: the control branch resident beside the UNet, and upstream ComfyUI's `ControlNet` object on top of it.

The reference keeps every seam of ControlNet and fills none: `apply_control1` returns `h` (LD.py:5290), `calc_cond_batch` carries `p.control`
and drops it (LD.py:2531-2541), `pre_run_control` is a stub (LD.py:2670).  Here the key has upstream's meaning, opt-in (`apply_control=True` on
the sampler entry points, sampling.py):

* `MI355XControlNet` owns the C handle (`ld_controlnet_create`: an `ld_unet` in control mode — upstream's cldm.ControlNet is the UNet's own
  time_embed / input_blocks / middle_block plus the hint encoder, the zero convolutions and middle_block_out), with the lifecycle of the other
  resident models.  `set_hint` encodes the control image once per run, `forward` / `forward_pair` leave the residuals in the handle.
* `ControlNet` is what a conditioning entry's "control" key holds: `set_cond_hint`, `copy`, `pre_run`, `get_models`,
  `inference_memory_requirements`, `cleanup` — the calls `get_models_from_cond` / `get_additional_models` / `cleanup_models` make
  (LD.py:2300-2340).

Out of scope, each refused with a plain message: chained ControlNets (`previous_controlnet`), T2I-Adapter / ControlLoRA / diffusers-layout
files, LoRA patches on the control branch.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import weights as W
from ._lib import ERR_SHAPE, FWD_PAIR, Control, LDError, check, lib
from ._model import WeightSource, _stream
from .unet import UNetHandle


def common_upscale(samples: torch.Tensor, width: int, height: int, upscale_method: str = "nearest-exact", crop: str = "center") -> torch.Tensor:
    """Upstream's comfy.utils.common_upscale for the modes the control hint uses: NCHW, a centre crop to the target's aspect ratio, then
    torch's interpolate."""
    if crop == "center":
        old_h, old_w = samples.shape[2], samples.shape[3]
        old_aspect, new_aspect = old_w / old_h, width / height
        x = y = 0
        if old_aspect > new_aspect:
            x = round((old_w - old_w * (new_aspect / old_aspect)) / 2)
        elif old_aspect < new_aspect:
            y = round((old_h - old_h * (old_aspect / new_aspect)) / 2)
        samples = samples[:, :, y:old_h - y, x:old_w - x]
    elif crop != "disabled":
        raise ValueError(f"crop must be 'center' or 'disabled', got {crop!r}")
    return torch.nn.functional.interpolate(samples, size=(height, width), mode=upscale_method)


class MI355XControlNet(UNetHandle):
    """The control branch of an SD1.x ControlNet resident on one MI355X.  `cfg`: the UNet config it was built on."""

    key_prefixes = ("", "control_model.")

    def __init__(self, cfg: dict, weights: WeightSource, hint_channels: int = 3, device="cuda:0", max_batch: int = 2, max_hw=(64, 64),
                 max_tokens: int = 77):
        self.cfg = dict(cfg)
        self.hint_channels = int(hint_channels)
        self.device = torch.device(device)
        c = self._config(cfg)
        self._ctx_token = None
        self.ctx_shape = None
        self.hint_shape = None           # (hb, h, w) of the resident encoded hint, latent units
        self.hint_epoch = 0              # bumped by every set_hint: captured graphs bake the hint's batch in
        self._create(weights, C.byref(c), self.hint_channels)
        self._reserve(max_batch, max_hw[0], max_hw[1], max_tokens)

    def _fn(self, op: str):
        return lib().ld_controlnet_create if op == "create" else super()._fn(op)

    def _workspace_moved(self) -> None:
        self._ctx_token = self.ctx_shape = self.hint_shape = None

    @property
    def residual_count(self) -> int:
        """residuals of a forward without the middle one: one per input block"""
        return lib().ld_controlnet_residual_count(self._h)

    def set_hint(self, image_nchw: torch.Tensor) -> None:
        """image_nchw [hb, hint_channels, 8 h, 8 w] in [0, 1]: encoded once (eight launches), resident until the workspace moves."""
        img = image_nchw.to(self.device, torch.float32).contiguous()
        hb, c, H, W = img.shape
        if c != self.hint_channels or H % 8 or W % 8:
            raise ValueError(f"control hint {tuple(img.shape)}: {self.hint_channels} channels and sides that are multiples of 8 expected")
        mn, _, _, mt = self._reserved
        self._ensure(hb, H // 8, W // 8, mt)
        with torch.cuda.device(self.device):
            check(lib().ld_controlnet_set_hint(self._h, img.data_ptr(), hb, H, W, _stream()), "ld_controlnet_set_hint")
        self.hint_shape = (hb, H // 8, W // 8)
        self.hint_epoch += 1

    def _run(self, x: torch.Tensor, sigma: torch.Tensor, *, pair: bool, profile: bool = False) -> None:
        """`ld_controlnet_forward` / `ld_controlnet_profile` behind the checks every public form shares: x [B,4,h,w] fp32, sigma [B] fp32 on the
        device, against the resident hint and the resident N-row context, N = 2B for a `pair`, else B.  The residuals stay in the handle."""
        assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and sigma.is_cuda and sigma.dtype == torch.float32 and sigma.is_contiguous()
        b, _, h, w = x.shape
        n = 2 * b if pair else b
        entry = "ld_controlnet_profile" if profile else "ld_controlnet_forward"
        mn, mh, mw, _ = self._reserved
        if n > mn or h > mh or w > mw:
            raise LDError(ERR_SHAPE, f"{entry}: input {n}x{h}x{w} exceeds the reserved plan {mn}x{mh}x{mw}")
        with torch.cuda.device(self.device):
            check(getattr(lib(), entry)(self._h, x.data_ptr(), sigma.data_ptr(), b, h, w, FWD_PAIR if pair else 0, _stream()), entry)

    def forward(self, x: torch.Tensor, sigma: torch.Tensor) -> None:
        """x [N,4,h,w] fp32, sigma [N] fp32 on the device, against the resident N-row context and hint: the residuals stay in the handle."""
        self._run(x, sigma, pair=False)

    def forward_pair(self, x: torch.Tensor, sigma: torch.Tensor) -> None:
        """The CFG pair of one step: x [B,4,h,w], sigma [B] against the 2B-row context: the residuals of `forward` on cat([x, x])."""
        self._run(x, sigma, pair=True)

    def profile(self, x: torch.Tensor, sigma: torch.Tensor) -> None:
        """`forward` with HIP events around every launch: `profile_launches()` is then the control branch's launch table."""
        self._run(x, sigma, pair=False, profile=True)

    def profile_pair(self, x: torch.Tensor, sigma: torch.Tensor) -> None:
        """`profile` of `forward_pair`: x [B,..], sigma [B]."""
        self._run(x, sigma, pair=True, profile=True)

    def hint(self) -> torch.Tensor:
        """A copy of the resident encoded hint, fp16 [hb, h, w, model_channels]."""
        hb, h, w, c = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        check(lib().ld_controlnet_read_hint(self._h, None, C.byref(hb), C.byref(h), C.byref(w), C.byref(c), None), "ld_controlnet_read_hint")
        t = torch.empty(hb.value, h.value, w.value, c.value, dtype=torch.float16, device=self.device)
        with torch.cuda.device(self.device):
            check(lib().ld_controlnet_read_hint(self._h, t.data_ptr(), None, None, None, None, _stream()), "ld_controlnet_read_hint")
        return t

    def control(self, strength: float, r_n: int = 0) -> Control:
        """The `ld_control` of the last forward's residuals (they live at fixed addresses until the workspace moves)."""
        ctl = Control()
        check(lib().ld_controlnet_fill_control(self._h, int(r_n), float(strength), C.byref(ctl)), "ld_controlnet_fill_control")
        return ctl

    def residuals(self) -> list:
        """Copies of the last forward's residuals, fp16 [N, H, W, C] each; the last one is the middle block's."""
        n = lib().ld_controlnet_residual_batch(self._h)
        out = []
        with torch.cuda.device(self.device):
            for i in range(self.residual_count + 1):
                p, c, h, w = C.c_void_p(), C.c_int(), C.c_int(), C.c_int()
                check(lib().ld_controlnet_residual(self._h, i, C.byref(p), C.byref(c), C.byref(h), C.byref(w)), "ld_controlnet_residual")
                t = torch.empty(n, h.value, w.value, c.value, dtype=torch.float16, device=self.device)
                check(lib().ld_controlnet_read_residual(self._h, i, t.data_ptr(), _stream()), "ld_controlnet_read_residual")
                out.append(t)
        return out


def synthetic_controlnet(cfg: Optional[dict] = None, seed: int = 0, hint_channels: int = 3, **kw) -> MI355XControlNet:
    cfg = cfg or W.sd15_unet_config()
    return MI355XControlNet(cfg, lambda name, shape: W.synth_controlnet_tensor(name, shape, seed), hint_channels=hint_channels, **kw)


class ControlNet:
    """Upstream's comfy.controlnet.ControlNet, the object a conditioning entry carries under "control": the resident control branch, the hint
    image, the strength and the share of the schedule it is active in.  `copy()` shares the resident model; each copy has its own hint."""

    def __init__(self, control_model: MI355XControlNet):
        self.control_model = control_model
        self.cond_hint_original = None
        self.strength = 1.0
        self.timestep_percent_range = (0.0, 1.0)
        self.timestep_range = None
        self.previous_controlnet = None
        self.encode_calls = 0            # hint encodes since construction (once per run)
        self._prepared = None            # (b, h, w) the resident hint was encoded for by THIS object

    def set_cond_hint(self, cond_hint: torch.Tensor, strength: float = 1.0, timestep_percent_range=(0.0, 1.0)):
        """cond_hint: NCHW [1 or B, hint_channels, H, W] in [0, 1], any size (resized to the latent's 8 h x 8 w once per run)."""
        self.cond_hint_original = cond_hint
        self.strength = float(strength)
        self.timestep_percent_range = (float(timestep_percent_range[0]), float(timestep_percent_range[1]))
        self._prepared = None
        return self

    def set_previous_controlnet(self, controlnet):
        if controlnet is not None:
            raise NotImplementedError("chained ControlNets (previous_controlnet) are not supported: apply one ControlNet to a conditioning")
        return self

    def copy(self):
        c = ControlNet(self.control_model)
        c.cond_hint_original, c.strength, c.timestep_percent_range = self.cond_hint_original, self.strength, self.timestep_percent_range
        return c

    def pre_run(self, model, percent_to_sigma_function):
        """Once per run: the percent range as sigmas, (sigma at start, sigma at end)."""
        self.timestep_range = (percent_to_sigma_function(self.timestep_percent_range[0]), percent_to_sigma_function(self.timestep_percent_range[1]))
        self._prepared = None

    @property
    def ranged(self) -> bool:
        """does the step range exclude any step?  (Only then does a step read sigma on the host.)"""
        return self.timestep_percent_range[0] > 0.0 or self.timestep_percent_range[1] < 1.0

    def get_models(self):
        return [self.control_model]

    def inference_memory_requirements(self, dtype=None) -> int:
        return int(self.control_model.workspace_bytes)

    def cleanup(self):
        self.timestep_range = None
        self._prepared = None

    def prepare(self, ctx: torch.Tensor, token, b: int, h: int, w: int) -> None:
        """Before a controlled step: the branch's context (once per run, by token) and its hint (once per run and latent shape)."""
        if self.cond_hint_original is None:
            raise ValueError("this ControlNet has no hint: ControlNetApply().apply_controlnet / set_cond_hint first")
        cm = self.control_model
        cm.sync_context(ctx, 2 * b, h, w, token)
        if self._prepared == (b, h, w, cm.reserve_epoch) and cm.hint_shape is not None and getattr(cm, "_hint_owner", None) is self:
            return
        hint = self.cond_hint_original
        if hint.shape[0] not in (1, b):
            raise ValueError(f"the control hint has batch {hint.shape[0]}; the latent batch is {b}: a hint batch of 1 or {b} is supported")
        hint = common_upscale(hint.to(cm.device, torch.float32), 8 * w, 8 * h, "nearest-exact", "center")
        cm.set_hint(hint)
        cm._hint_owner = self
        self.encode_calls += 1
        self._prepared = (b, h, w, cm.reserve_epoch)
