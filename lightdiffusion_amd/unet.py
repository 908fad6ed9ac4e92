"""MI355X UNet / VAE objects that sit behind the reference's plugin seams.

* `MI355XUNet` satisfies the `model_function_wrapper` contract (LD.py:2558-2567, installed with
  `ModelPatcher.set_model_unet_function_wrapper`, LD.py:3277): `fn(apply_model, {"input", "timestep", "c",
  "cond_or_uncond"}) -> denoised fp32`, plus `.to(device)` (LD.py:3286-3291) — the same contract the reference's
  stable-fast integration implements (`StableFastPatch`, LD.py:9902-9933).
* `MI355XVAE.decode` mirrors `VAE.decode` (LD.py:6357-6381): [B,4,h,w] -> [B,8h,8w,3] fp32 in [0,1].

Both are thin: they own a C handle, feed it device pointers and the current HIP stream.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional

import torch

from . import weights as W
from ._lib import ERR_SHAPE, F16, F32, FWD_EPS_ONLY, FWD_PAIR, LDError, LoraTerm, UNetConfig, VAEConfig, check, lib
from ._model import ResidentModel, WeightSource, _stream


def lora_factor_mismatch(shape, up, down) -> Optional[str]:
    """Why the LoRA factors (up, down) cannot patch a weight of `shape` (checkpoint layout), or None when they fit: the patched matrix is
    [shape[0]][prod(shape[1:])] (calculate_weight, LD.py:3420), so up flattens to [shape[0]][rank] and down to [rank][prod(shape[1:])]."""
    if len(shape) < 2 or up.dim() < 2 or down.dim() < 2:
        return f"weight {tuple(shape)}, up {tuple(up.shape)}, down {tuple(down.shape)}: not matrices"
    rows, cols = int(shape[0]), math.prod(int(d) for d in shape[1:])
    got = (up.shape[0], math.prod(up.shape[1:]), down.shape[0], math.prod(down.shape[1:]))
    if got[0] != rows or got[3] != cols or got[1] != got[2]:
        return f"up {tuple(up.shape)} x down {tuple(down.shape)} is not a [{rows}][{cols}] update of a weight of shape {tuple(shape)}"
    return None


def lora_terms(terms, device, shape):
    """[(up, down, scale), ...] -> (ctypes array of ld_lora_term, tensors to keep alive until the merge is queued).  Plumbing only: the
    factors go to the device as [rows][rank] / [rank][cols] row-major (a conv's down as flatten(start_dim=1), calculate_weight LD.py:3420),
    fp16 or fp32 as they come; the arithmetic is the kernel's.  `shape` is the patched weight's, in checkpoint layout: the C calls take raw
    pointers and index them by the SLOT's rows and columns, so factors of any other size are refused here (ValueError)."""
    arr = (LoraTerm * len(terms))()
    keep = []
    for j, (up, down, scale) in enumerate(terms):
        why = lora_factor_mismatch(shape, up, down)
        if why is not None:
            raise ValueError("LoRA factors do not fit: " + why)
        dt = torch.float16 if up.dtype == torch.float16 and down.dtype == torch.float16 else torch.float32
        up = up.flatten(start_dim=1).to(device, dt).contiguous()
        down = down.flatten(start_dim=1).to(device, dt).contiguous()
        keep += [up, down]
        arr[j].up, arr[j].down = up.data_ptr(), down.data_ptr()
        arr[j].dtype, arr[j].rank, arr[j].scale = (F16 if dt == torch.float16 else F32), up.shape[1], float(scale)
    return arr, keep


class UNetHandle(ResidentModel):
    """What the two owners of an `ld_unet` handle share — `MI355XUNet` and `controlnet.MI355XControlNet`, whose control branch is an `ld_unet`
    in control mode: the config, the sizes, the parameters read back, the resident context and the per-run token that says whose it is."""

    family, reserve_rank = "unet", 4

    @staticmethod
    def _config(cfg: dict) -> UNetConfig:
        """`ld_unet_config` of a cfg dict as in `weights.sd15_unet_config()` (a control branch has no `transformer_depth_output`)."""
        c = UNetConfig()
        c.in_channels, c.out_channels, c.model_channels = cfg["in_channels"], cfg["out_channels"], cfg["model_channels"]
        c.num_levels = len(cfg["channel_mult"])
        for field in ("channel_mult", "num_res_blocks", "transformer_depth", "transformer_depth_output"):
            for i, v in enumerate(cfg.get(field, ()) if field == "transformer_depth_output" else cfg[field]):
                getattr(c, field)[i] = v
        c.transformer_depth_middle = cfg["transformer_depth_middle"]
        c.context_dim, c.num_heads = cfg["context_dim"], cfg["num_heads"]
        return c

    @property
    def weight_bytes(self) -> int:
        """Resident weights and the copies derived from them.  The backups of LoRA-patched slots are a further resident copy, held only
        while a patch is applied and reported separately: `patch_bytes`."""
        return lib().ld_unet_weight_bytes(self._h)

    def read_param(self, name: str) -> torch.Tensor:
        """The resident value of one parameter, back in checkpoint layout (fp16, device)."""
        shapes = self.param_shapes()
        if name not in shapes:
            raise KeyError(name)
        out = torch.empty(shapes[name], dtype=torch.float16, device=self.device)
        with torch.cuda.device(self.device):
            check(lib().ld_unet_read_param(self._h, name.encode(), out.data_ptr(), _stream()), f"ld_unet_read_param({name})")
        return out

    def set_context(self, ctx: torch.Tensor) -> None:
        """ctx [N, T, context_dim], in the batch order of the forwards that follow, exactly as the reference batches it: [uncond..., cond...]."""
        ctx = ctx.to(self.device)
        if ctx.dtype not in (torch.float16, torch.float32):
            ctx = ctx.float()
        ctx = ctx.contiguous()
        _, mh, mw, _ = self._reserved
        self._ensure(ctx.shape[0], mh, mw, ctx.shape[1])
        with torch.cuda.device(self.device):
            check(lib().ld_unet_set_context(self._h, ctx.data_ptr(), F32 if ctx.dtype == torch.float32 else F16, ctx.shape[0],
                                            ctx.shape[1], _stream()), "ld_unet_set_context")
        self._ctx_token = None
        self.ctx_shape = (ctx.shape[0], ctx.shape[1])

    def _ctx_current(self, ctx: torch.Tensor, n: int, h: int, w: int, token) -> bool:
        """Grows the workspace to the call; then: is the resident context this run's, by the never-reused per-run token of our own sampling
        stack (sampling.sampling_function)?"""
        self._ensure(n, h, w, ctx.shape[1])
        return token is not None and token == self._ctx_token and self.ctx_shape == (ctx.shape[0], ctx.shape[1])

    def sync_context(self, ctx: torch.Tensor, n: int, h: int, w: int, token) -> None:
        """The context of a run, by its token: projected once per run.  (A control branch: call it before `set_hint` — growing the workspace
        drops the hint.)"""
        if not self._ctx_current(ctx, n, h, w, token):
            self.set_context(ctx)
            self._ctx_token = token


class MI355XUNet(UNetHandle):
    """SD1.x UNet resident on one MI355X.  `cfg` as in `weights.sd15_unet_config()`."""

    key_prefixes = ("", "model.diffusion_model.")

    def __init__(self, cfg: dict, weights: WeightSource, device="cuda:0", max_batch: int = 2, max_hw=(64, 64), max_tokens: int = 77):
        self.cfg = dict(cfg)
        self.device = torch.device(device)
        c = self._config(cfg)
        self._create(weights, C.byref(c))
        self.reserve(max_batch, max_hw, max_tokens)
        self._ctx_ref = None             # device copy of the context the resident K / V^T were projected from
        self._ctx_token = None           # per-run token of our own sampling stack (sampling.sampling_function)
        self.ctx_shape = None            # (n, tokens) of the resident context
        self._denoisers = {}
        self.hook_graph = True           # the wrapper hook replays captured hipGraphs (False: eager launches, for A/B tests)
        self._hook = {}                  # (N, h, w) -> pipeline.HookRunner
        self._hook_flags = None          # pinned host ints the device-side guards write (ld_op_hook_check)
        self._hook_event = None
        self._hook_epoch = 0
        self.applied_patches_uuid = None  # identity of the LoRA patch set merged into the resident weights (None: the loaded weights)

    def reserve(self, max_batch: int, max_hw=(64, 64), max_tokens: int = 77) -> None:
        """(Re)size the activation workspace.  Growing it frees and reallocates: the context must be set again and every
        captured graph is stale (`reserve_epoch`)."""
        self._reserve(max_batch, max_hw[0], max_hw[1], max_tokens)

    def _workspace_moved(self) -> None:
        self._ctx_ref = self._ctx_token = self.ctx_shape = None
        self._denoisers = {}
        self._hook = {}

    # -- sizes
    @property
    def patch_bytes(self) -> int:
        return lib().ld_unet_patch_bytes(self._h)

    # -- parameters and LoRA patches of the resident weights
    def _weights_changed(self) -> None:
        """After a patch / unpatch: re-derive the folded copies now (a replayed hipGraph never runs the executor's own check) and forget
        the resident context — the hoisted cross-attention K / V^T were projected with attn2.to_k / to_v, so the next call re-projects them
        whatever token or content it carries.  Workspaces, `reserve_epoch` and captured graphs stay: no address moves."""
        with torch.cuda.device(self.device):
            check(lib().ld_unet_refresh_derived(self._h, _stream()), "ld_unet_refresh_derived")
        self._ctx_ref = self._ctx_token = None

    def patch_weights(self, patches: Dict[str, list], uuid=None) -> None:
        """ModelPatcher.patch_model (LD.py:3335-3354) on the resident weights: `patches` {parameter name: [(up, down, scale), ...]}; every
        slot becomes round_fp16(loaded weight + sum scale up down) (`ld_unet_patch_param`).  Whatever was patched before is restored first, so
        the result never depends on the previous patch set.  A patch that is refused (an unknown name, factors that do not fit the weight,
        a rank or a number of terms out of range) raises, and leaves the loaded weights in place."""
        shapes = self.param_shapes()
        with torch.cuda.device(self.device):
            check(lib().ld_unet_unpatch(self._h, None, _stream()), "ld_unet_unpatch")
            try:
                for name, terms in patches.items():
                    if name not in shapes:
                        raise KeyError(f"the UNet has no parameter '{name}'")
                    arr, keep = lora_terms(terms, self.device, shapes[name])
                    check(lib().ld_unet_patch_param(self._h, name.encode(), arr, len(terms), _stream()), f"ld_unet_patch_param({name})")
                    del keep
            except Exception:
                check(lib().ld_unet_unpatch(self._h, None, _stream()), "ld_unet_unpatch")
                self.applied_patches_uuid = None
                self._weights_changed()
                raise
        self.applied_patches_uuid = uuid if uuid is not None else object()   # (a direct call: matches no patcher, so the next lazy swap restores)
        self._weights_changed()

    def unpatch_weights(self, uuid=None) -> None:
        """ModelPatcher.unpatch_model (LD.py:3426-3437): the loaded weights back, bit for bit.  `uuid`: the identity recorded as applied
        (a patcher whose patch set is empty)."""
        changed = self.patch_bytes > 0
        with torch.cuda.device(self.device):
            check(lib().ld_unet_unpatch(self._h, None, _stream()), "ld_unet_unpatch")
        self.applied_patches_uuid = uuid
        if changed:
            self._weights_changed()

    # -- hot path
    def set_context(self, ctx: torch.Tensor) -> None:
        super().set_context(ctx)
        self._ctx_ref = None

    KERNEL_CLASSES = ("conv3x3", "gemm", "attention", "groupnorm", "layernorm", "misc")

    def _run(self, x: torch.Tensor, sigma: torch.Tensor, *, pair: bool, control=None, out: Optional[torch.Tensor] = None, eps_only: bool = False,
             profile: bool = False):
        """`ld_unet_forward` / `ld_unet_profile` behind the checks every public form shares.  x [B,4,h,w] fp32 and sigma [B] fp32 on the device;
        the batch that runs and is written is N = 2B for a `pair`, else B.  `control`: an `_lib.Control` (e.g. MI355XControlNet.control()) whose
        residuals are added to the skip tensors and the middle block's output in one launch behind the middle block, or None.  Returns `out`
        [N,4,h,w], or with `profile` (HIP events around every launch) {class: (ms, flops, launches)}."""
        assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
        assert sigma.is_cuda and sigma.dtype == torch.float32 and sigma.is_contiguous()
        b, c, h, w = x.shape
        n = 2 * b if pair else b
        entry = "ld_unet_profile" if profile else "ld_unet_forward"
        mn, mh, mw, _ = self._reserved
        if n > mn or h > mh or w > mw:
            raise LDError(ERR_SHAPE, f"{entry}: input {n}x{h}x{w} exceeds the reserved plan {mn}x{mh}x{mw} (reserve(), then set_context)")
        if out is None:
            out = torch.empty(n, c, h, w, dtype=torch.float32, device=x.device)
        args = (self._h, x.data_ptr(), sigma.data_ptr(), out.data_ptr(), b, h, w, (FWD_PAIR if pair else 0) | (FWD_EPS_ONLY if eps_only else 0),
                None if control is None else C.byref(control), _stream())
        with torch.cuda.device(self.device):
            if not profile:
                check(lib().ld_unet_forward(*args), entry)
                return out
            ms, fl, nl = (C.c_double * 6)(), (C.c_double * 6)(), (C.c_int * 6)()
            check(lib().ld_unet_profile(*args, ms, fl, nl), entry)
        return {k: (ms[i], fl[i], nl[i]) for i, k in enumerate(self.KERNEL_CLASSES)}

    def forward(self, x: torch.Tensor, sigma: torch.Tensor, out: Optional[torch.Tensor] = None, eps_only: bool = False, control=None) -> torch.Tensor:
        """x [N,4,h,w] fp32 (device), sigma [N] fp32 (device) -> denoised [N,4,h,w] fp32 = x - eps*sigma."""
        return self._run(x, sigma, pair=False, control=control, out=out, eps_only=eps_only)

    def forward_pair(self, x: torch.Tensor, sigma: torch.Tensor, out: Optional[torch.Tensor] = None, control=None) -> torch.Tensor:
        """The classifier-free-guidance pair of one sampler step (calc_cond_batch's cat([x, x]) against cat([uncond, cond]), LD.py:2515-2547):
        x [B,4,h,w], sigma [B] -> denoised [2B,4,h,w] in the order [uncond.., cond..] of the resident 2B-row context.  The layers in front of
        the first cross-attention are evaluated once for both halves (`LD_FWD_PAIR`)."""
        return self._run(x, sigma, pair=True, control=control, out=out)

    def profile(self, x: torch.Tensor, sigma: torch.Tensor, control=None) -> dict:
        """One forward with HIP events around every launch; returns {class: (ms, flops, launches)}."""
        return self._run(x, sigma, pair=False, control=control, profile=True)

    def profile_pair(self, x: torch.Tensor, sigma: torch.Tensor, control=None) -> dict:
        """`profile` of the CFG-pair route (`forward_pair`): x [B,..], sigma [B]."""
        return self._run(x, sigma, pair=True, control=control, profile=True)

    def profile_kernels(self) -> dict:
        """Per kernel instantiation of the last `profile()` call: {name: (ms, flops, launches)}."""
        buf = C.create_string_buffer(1 << 16)
        check(lib().ld_unet_profile_kernels(self._h, buf, len(buf)), "ld_unet_profile_kernels")
        out = {}
        for line in buf.value.decode().splitlines():
            name, n, ms, fl = line.split("\t")
            out[name] = (float(ms), float(fl), int(n))
        return out

    # -- the reference's plugin seam
    def _sync_context(self, ctx: torch.Tensor, n: int, h: int, w: int, token=None) -> None:
        """Make the resident cross-attention K / V^T those of `ctx`.  The reference re-concatenates the context every step
        (cond_cat, LD.py:2471-2489) into a fresh tensor whose address the caching allocator recycles, so identity proves
        nothing: the CONTENT is compared with the device copy of what was projected (one small elementwise kernel + a host
        read per call).  Our own sampling stack passes a never-reused per-run `token` instead and skips the comparison."""
        if self._ctx_current(ctx, n, h, w, token):
            return
        c = ctx.to(self.device)
        same = self._ctx_ref is not None and self._ctx_ref.shape == c.shape and self._ctx_ref.dtype == c.dtype and torch.equal(c, self._ctx_ref)
        if not same:
            self.set_context(c)
            with torch.inference_mode(False):          # (a plain tensor: the wrapper hook may update it in place later, in either mode)
                self._ctx_ref = c.clone()
        self._ctx_token = token

    def __call__(self, apply_model, params: dict) -> torch.Tensor:
        """The `model_function_wrapper` contract (LD.py:2558-2567): returns the denoised batch, fp32, in the caller's batch order.

        Every call replays a captured hipGraph on static buffers (`pipeline.HookRunner`; the reference's plugin on this seam has the
        same option, `enable_cuda_graph`, LD.py:9896-9933).  When the caller batched one latent against [uncond, cond]
        (`cond_or_uncond == [1, 0]`: what `calc_cond_batch` builds, LD.py:2515-2547) the CFG-pair graph is replayed — SPECULATIVELY:
        whether the two halves of `input` / `timestep` really are the same tensors, and whether `c_crossattn` still holds the
        conditioning the resident cross-attention K / V^T were projected from, is checked on the device (`ld_op_hook_check`) into
        pinned host flags that are read only after the replay has been queued.  A failed guess (a new prompt, halves that differ)
        re-projects the context and / or replays the plain graph before the result is handed back, so the GPU never idles for the check
        and the result is always that of the plain forward on these inputs (up to the pair route's tile rounding)."""
        x = params["input"].to(self.device, torch.float32).contiguous()
        sigma = params["timestep"].to(self.device, torch.float32).contiguous()
        ctx = params["c"]["c_crossattn"]
        topt = params["c"].get("transformer_options") or {}
        token = topt.get("ld_ctx_token")
        if token is not None or not self.hook_graph:
            # our own sampling stack's un-fused route (`ld_eager_unbatched`): per-run token instead of a content check, eager launches
            self._sync_context(ctx, x.shape[0], x.shape[2], x.shape[3], token)
            return self.forward(x, sigma)
        return self._hook_replay(x, sigma, ctx, params.get("cond_or_uncond"))

    def _hook_replay(self, x: torch.Tensor, sigma: torch.Tensor, ctx: torch.Tensor, cond_or_uncond) -> torch.Tensor:
        from .pipeline import HookRunner
        n, _, h, w = x.shape
        c = ctx.to(self.device)
        if c.dtype not in (torch.float16, torch.float32):
            c = c.float()
        c = c.contiguous()
        self._ensure(n, h, w, c.shape[1])
        known = self._ctx_ref is not None and self._ctx_ref.shape == c.shape and self._ctx_ref.dtype == c.dtype
        if not known:                                  # first call, or another number of tokens / rows: nothing to speculate on
            self.set_context(c)
            with torch.inference_mode(False):          # (a plain tensor: later calls update it in place, inside or outside inference mode)
                self._ctx_ref = c.clone()
        key = (n, h, w)
        run = self._hook.get(key)
        if run is None:
            if len(self._hook) >= 4:
                self._hook.pop(next(iter(self._hook)))
            run = self._hook[key] = HookRunner(self, n, h, w)
        if self._hook_flags is None:
            with torch.inference_mode(False):
                self._hook_flags = torch.zeros(2, dtype=torch.int32).pin_memory()
            self._hook_event = torch.cuda.Event()
        pair = run.pair is not None and cond_or_uncond is not None and list(cond_or_uncond) == [1, 0] and not run.halves_differed
        self._hook_epoch += 1
        run.x.copy_(x)
        run.sigma.copy_(sigma)
        half = n // 2
        with torch.cuda.device(self.device):
            check(lib().ld_op_hook_check(c.data_ptr() if known else None, self._ctx_ref.data_ptr() if known else None,
                                         c.numel() * c.element_size() // 4 if known else 0,
                                         run.x.data_ptr() if pair else None, run.x.numel() // 2 if pair else 0,
                                         run.sigma.data_ptr() if pair else None, half if pair else 0,
                                         self._hook_flags.data_ptr(), self._hook_epoch, _stream()), "ld_op_hook_check")
        self._hook_event.record()
        (run.pair if pair else run.plain).launch()     # speculative: queued before the flags are looked at
        self._hook_event.synchronize()                 # waits for the check kernel only; the replay behind it keeps the GPU busy
        ctx_changed = known and int(self._hook_flags[0]) == self._hook_epoch
        halves_differ = pair and int(self._hook_flags[1]) == self._hook_epoch
        if ctx_changed:
            ref = self._ctx_ref
            self.set_context(c)                        # (clears the reference: it no longer describes the resident projections)
            ref.copy_(c)
            self._ctx_ref = ref
        if halves_differ:
            run.halves_differed = True                 # this caller does not batch one latent twice: stay on the plain graph
        if ctx_changed or halves_differ:
            (run.plain if halves_differ or not pair else run.pair).launch()
        return run.out.clone()

    def cfg_denoise(self, x: torch.Tensor, timestep: torch.Tensor, ctx: torch.Tensor, cond_scale: float, token=None,
                    use_graph: bool = True, control=None) -> torch.Tensor:
        """One classifier-free-guided step (sampling_function, LD.py:2609-2626) through a cached, hipGraph-captured
        `pipeline.CFGDenoiser`: ctx is the [uncond.., cond..] batch (2B rows), x [B,4,h,w], timestep [B] (sigma) on the device.
        This is what `KSampler2.sample` reaches through `sampling.sampling_function`; the reference's counterpart is the
        CUDA-graph option of its stable-fast patch (LD.py:9902-9946).
        `control`: a controlnet.ControlNet whose branch runs on the same [uncond, cond] batch and context in front of the UNet, inside the
        same captured step; the denoiser is keyed by the resident control model and the strength as well."""
        from .pipeline import CFGDenoiser
        b, _, h, w = x.shape
        x = x.to(self.device, torch.float32)
        self._sync_context(ctx, 2 * b, h, w, token)
        key = (b, h, w, float(cond_scale), bool(use_graph))
        if control is not None:
            control.prepare(ctx, token, b, h, w)
            key += (id(control.control_model), float(control.strength))
        d = self._denoisers.get(key)
        if d is None:
            if len(self._denoisers) >= 4:                      # a few shapes per session (txt2img + hires pass); drop the oldest
                self._denoisers.pop(next(iter(self._denoisers)))
            d = self._denoisers[key] = CFGDenoiser(self, b, h, w, cond_scale, use_graph=use_graph,
                                                   control=None if control is None else (control.control_model, float(control.strength)))
        return d.run(x, timestep.to(self.device, torch.float32)).clone()   # samplers keep `denoised` across steps (old_denoised)

    def to(self, device):
        """LD.py:3286-3291 calls this on load / unload.  The weights stay resident (they are not torch tensors); like the reference's
        graph-mode plugin (StableFastPatch.to, LD.py:9921-9933) an unload to the CPU drops the captured graphs and their static buffers."""
        if torch.device(device).type == "cpu":
            self._denoisers = {}
            self._hook = {}
        return self


class MI355XVAE(ResidentModel):
    """KL-VAE decoder resident on one MI355X.  `cfg` as in `weights.sd15_vae_config()`."""

    family, key_prefixes = "vae", ("", "first_stage_model.")
    downscale_ratio = 8
    latent_channels = 4

    def __init__(self, cfg: dict, weights: WeightSource, device="cuda:0", max_batch: int = 1, max_hw=(64, 64), with_encoder: bool = False):
        self.cfg = dict(cfg)
        self.device = torch.device(device)
        self.with_encoder = bool(with_encoder)
        c = VAEConfig()
        c.with_encoder = int(self.with_encoder)
        c.z_channels, c.ch, c.num_levels = cfg["z_channels"], cfg["ch"], len(cfg["ch_mult"])
        for i, v in enumerate(cfg["ch_mult"]):
            c.ch_mult[i] = v
        c.num_res_blocks, c.out_ch = cfg["num_res_blocks"], cfg["out_ch"]
        self._create(weights, C.byref(c))
        self._ensure(max_batch, max_hw[0], max_hw[1])

    memory_fraction = 0.9          # share of the free device memory a decode's workspace may take
    memory_budget = None           # bytes; None: ask the driver (torch.cuda.mem_get_info) — tests set it to force the split

    def batch_number(self, b: int, h: int, w: int) -> int:
        """VAE.decode's split of the batch by free memory (LD.py:6357-6362: batch_number = free_memory / memory_used): the largest slice
        of the batch whose planned workspace (`ld_vae_plan_bytes`, a host-only dry run of the executor) fits the budget; at least 1."""
        mb, mh, mw = self._reserved
        if b <= mb and h <= mh and w <= mw:
            return b                                              # fits the workspace that is already there
        budget = self.memory_budget
        if budget is None:
            free, _ = torch.cuda.mem_get_info(self.device)
            budget = self.memory_fraction * (free + (self.workspace_bytes if any(self._reserved) else 0))   # (a re-reserve frees the old one first)
        _, ph, pw = self._grown(b, h, w)                          # (the sizes `_ensure` will reserve)
        n = b
        while n > 1:
            need = self.plan_bytes(n, ph, pw)
            if 0 < need <= budget:
                break
            n = (n + 1) // 2
        return n

    def decode_device(self, z: torch.Tensor) -> torch.Tensor:
        z = z.to(self.device, torch.float32).contiguous()
        b, _, h, w = z.shape
        n = self.batch_number(b, h, w)
        self._ensure(n, h, w)
        out = torch.empty(b, 8 * h, 8 * w, self.cfg["out_ch"], dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            for x in range(0, b, n):                              # (one slice when everything fits: the usual case with 288 GB)
                m = min(n, b - x)
                check(lib().ld_vae_decode(self._h, z[x:x + m].data_ptr(), out[x:x + m].data_ptr(), m, h, w, _stream()), "ld_vae_decode")
        return out

    def profile_decode(self, z: torch.Tensor) -> list:
        """One decode with HIP events around every launch -> [(what, dims, flops, microseconds, kernel)] in launch order."""
        z = z.to(self.device, torch.float32).contiguous()
        b, _, h, w = z.shape
        self._ensure(b, h, w)
        out = torch.empty(b, 8 * h, 8 * w, self.cfg["out_ch"], dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            check(lib().ld_vae_profile(self._h, z.data_ptr(), out.data_ptr(), b, h, w, _stream()), "ld_vae_profile")
        return self.profile_launches()

    def profile_encode(self, pixel_samples: torch.Tensor) -> list:
        """One encode_moments with HIP events around every launch -> the launch table, as profile_decode."""
        px, (b, h, w) = self._encoder_input(pixel_samples)
        out = torch.empty(b, 2 * self.cfg["z_channels"], h, w, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            check(lib().ld_vae_profile_encode(self._h, px.data_ptr(), out.data_ptr(), b, h, w, _stream()), "ld_vae_profile_encode")
        return self.profile_launches()

    def decode(self, samples_in: torch.Tensor) -> torch.Tensor:
        """VAE.decode (LD.py:6357-6381): returns [B, 8h, 8w, 3] fp32 in [0,1] on the CPU (`intermediate_device`)."""
        return self.decode_device(samples_in).cpu()

    def _encoder_input(self, pixel_samples: torch.Tensor):
        """pixels [B, H, W, 3] in [0,1] -> (fp32 NCHW in [-1, 1] on the device, (B, H/8, W/8)), the workspace grown to that shape."""
        if not self.with_encoder:
            raise RuntimeError("this MI355XVAE was created without the encoder (with_encoder=True)")
        px = pixel_samples[..., :3].to(self.device, torch.float32).movedim(-1, 1)
        px = (px * 2.0 - 1.0).contiguous()                                   # process_input, LD.py:6295
        b, _, H, W = px.shape
        h, w = H // 8, W // 8
        if h * 8 != H or w * 8 != W:
            raise ValueError("image sides must be multiples of 8")
        self._ensure(b, h, w)
        return px, (b, h, w)

    def encode_moments(self, pixel_samples: torch.Tensor) -> torch.Tensor:
        """pixels [B, H, W, 3] in [0,1] -> moments [B, 2z, H/8, W/8] fp32 on the device (mean | logvar): everything of
        VAE.encode (LD.py:6383-6410) up to, but excluding, the regularizer's random sample."""
        px, (b, h, w) = self._encoder_input(pixel_samples)
        out = torch.empty(b, 2 * self.cfg["z_channels"], h, w, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            check(lib().ld_vae_encode(self._h, px.data_ptr(), out.data_ptr(), b, h, w, _stream()), "ld_vae_encode")
        return out

    def encode(self, pixel_samples: torch.Tensor) -> torch.Tensor:
        """VAE.encode (LD.py:6383-6410): [B,H,W,3] in [0,1] -> latent [B,4,H/8,W/8] fp32 on the CPU.  The posterior sample
        (DiagonalGaussianDistribution.sample, LD.py:175-179) draws torch.randn on the HOST global generator, as the reference does."""
        m = self.encode_moments(pixel_samples).cpu()
        mean, logvar = torch.chunk(m, 2, dim=1)
        std = torch.exp(0.5 * torch.clamp(logvar, -30.0, 20.0))
        return mean + std * torch.randn(mean.shape)


def synthetic_unet(cfg: Optional[dict] = None, seed: int = 0, **kw) -> MI355XUNet:
    cfg = cfg or W.sd15_unet_config()
    return MI355XUNet(cfg, lambda name, shape: W.synth_tensor(name, shape, seed), **kw)


def synthetic_vae(cfg: Optional[dict] = None, seed: int = 0, **kw) -> MI355XVAE:
    cfg = cfg or W.sd15_vae_config()
    return MI355XVAE(cfg, lambda name, shape: W.synth_tensor(name, shape, seed), **kw)
