"""The reference's workflow-node call surface (LD.py:6573-6725, call order of `pipeline()` LD.py:10001-10086),
backed by the MI355X hot path.  A user of the reference keeps writing

    model, clip, vae = CheckpointLoaderSimple().load_checkpoint(path)
    pos = CLIPTextEncode().encode(clip, "a cat")[0];  neg = CLIPTextEncode().encode(clip, "")[0]
    lat = EmptyLatentImage().generate(512, 512, 1)[0]
    lat = KSampler2().sample(model, seed, 20, 7.0, "dpmpp_2m_sde", "karras", pos, neg, lat)[0]
    img = VAEDecode().decode(vae, lat)[0]

and gets the HIP UNet / VAE underneath.  The UNet is attached through the reference's own plugin seam:
`ModelPatcher.set_model_unet_function_wrapper` (LD.py:3277).
"""
from __future__ import annotations

import copy
import os
from typing import Optional

import torch

from . import sampling
from . import weights as W
from .clip import CLIP, CLIPTextModelHIP, LoraPatches, PromptTokenizer, _add_patches, patch_terms
from .detailer import DifferentialDiffusion  # noqa: F401  (a node of the reference's: apply / forward, LD.py:8945-8965)
from .preview import LatentPreviewer, MI355XTAESD
from .sampling import LATENT_SCALE, common_ksampler
from .unet import MI355XUNet, MI355XVAE
from .upscale import MI355XUpscaler, tiled_upscale


class SD15LatentFormat:
    """LatentFormat / SD15 (LD.py:125-147)."""
    scale_factor = LATENT_SCALE

    def process_in(self, latent):
        return latent * self.scale_factor

    def process_out(self, latent):
        return latent / self.scale_factor


class SD15Model:
    """The slice of BaseModel (LD.py:5798-5897) the sampling stack touches."""

    def __init__(self, unet: MI355XUNet):
        self.diffusion_model = unet
        self.model_sampling = sampling.ModelSampling()
        self.latent_format = SD15LatentFormat()
        self.lora = None                 # the LoraPatches of the ModelPatcher this view of the resident UNet belongs to (shared with it)

    def apply_model(self, x, t, c_crossattn=None, transformer_options=None, **kwargs):
        """BaseModel.apply_model (LD.py:5828-5860) — routed through the same wrapper object the hook would call, with the LoRA patches
        of the patcher this view belongs to swapped in first (clones share the resident UNet)."""
        if self.lora is not None:
            _swap_unet_patches(self.diffusion_model, self.lora)
        return self.diffusion_model(None, {"input": x, "timestep": t, "c": {"c_crossattn": c_crossattn}, "cond_or_uncond": [1, 0]})

    def process_latent_in(self, latent):
        return self.latent_format.process_in(latent)

    def process_latent_out(self, latent):
        return self.latent_format.process_out(latent)


def _swap_unet_patches(unet, lora: LoraPatches) -> None:
    """Lazy swap: nothing when the resident weights already carry these patches (one uuid comparison); an empty set restores the loaded
    weights."""
    if getattr(unet, "applied_patches_uuid", None) == lora.uuid:
        return
    if lora.patches:
        unet.patch_weights({k[len(ModelPatcher.KEY_PREFIX):]: patch_terms(v) for k, v in lora.patches.items()}, lora.uuid)
    else:
        unet.unpatch_weights(lora.uuid)


class ModelPatcher:
    """ModelPatcher (LD.py:3210-3437), reduced to what the hot path uses: model_options, the UNet wrapper hook, and LoRA weight patches
    (add_patches / patch_model / unpatch_model, LD.py:3297-3354, 3426-3437).  The weights live once, resident in the MI355XUNet that every
    clone shares; a clone carries its own patch LIST, and `patch_model` makes the resident weights those of this clone when they are not.
    Every patcher has an `SD15Model` view of its own on the resident UNet (`clone().model is not model`; the UNet, the sigma table and the
    latent format are shared): the view and the patcher hold the SAME `LoraPatches` object, so `model.apply_model` swaps in the right
    patches whichever of the two outlives the other.  A patcher built on a view that already belongs to another one takes a copy."""

    KEY_PREFIX = "model.diffusion_model."

    def __init__(self, model: SD15Model, load_device, offload_device=None):
        self._lora = LoraPatches()
        if isinstance(model, SD15Model):
            if model.lora is not None:
                model = copy.copy(model)
            model.lora = self._lora
        self.model = model
        self.load_device = torch.device(load_device)
        self.offload_device = offload_device
        self.model_options = {"transformer_options": {}}

    # checkpoint key -> [(strength_patch, (up, down, alpha), strength_model)], and the identity of that set (None: the loaded weights)
    patches = property(lambda self: self._lora.patches, lambda self, v: setattr(self._lora, "patches", v))
    patches_uuid = property(lambda self: self._lora.uuid, lambda self, v: setattr(self._lora, "uuid", v))

    def clone(self):
        n = ModelPatcher(self.model, self.load_device, self.offload_device)
        n.model_options = copy.copy(self.model_options)
        n.patches = {k: list(v) for k, v in self.patches.items()}
        n.patches_uuid = self.patches_uuid
        return n

    def model_key_shapes(self):
        """{checkpoint key: shape} of the UNet's parameters"""
        return {self.KEY_PREFIX + k: s for k, s in self.model.diffusion_model.param_shapes().items()}

    def add_patches(self, patches, strength_patch=1.0, strength_model=1.0):
        return _add_patches(self, self.model_key_shapes(), patches, strength_patch, strength_model)

    def patch_model(self, device_to=None, patch_weights=True):
        """Lazy swap: nothing when the resident weights already carry this patcher's patches; an empty set restores the loaded weights."""
        if patch_weights:
            _swap_unet_patches(self.model.diffusion_model, self._lora)
        return self.model

    def unpatch_model(self, device_to=None, unpatch_weights=True):
        if unpatch_weights:
            self.model.diffusion_model.unpatch_weights()

    def set_model_unet_function_wrapper(self, unet_wrapper_function):
        self.model_options["model_function_wrapper"] = unet_wrapper_function

    def set_model_denoise_mask_function(self, denoise_mask_function):
        """LD.py:3280-3281.  Kept across clone() with the rest of model_options; the reference's sampler never calls it (detailer.py)."""
        self.model_options["denoise_mask_function"] = denoise_mask_function

    def get_model_object(self, name):
        return getattr(self.model, name)

    def model_patches_to(self, device):
        w = self.model_options.get("model_function_wrapper")
        if w is not None and hasattr(w, "to"):
            self.model_options["model_function_wrapper"] = w.to(device)


# ------------------------------------------------------------------ nodes
class EmptyLatentImage:
    def generate(self, width, height, batch_size=1):
        return ({"samples": torch.zeros([batch_size, 4, height // 8, width // 8])},)


class CLIPTextEncode:
    def encode(self, clip: CLIP, text: str):
        cond, pooled = clip.encode_from_tokens(clip.tokenize(text), return_pooled=True)
        return ([[cond, {"pooled_output": pooled}]],)


class CLIPSetLastLayer:
    def set_last_layer(self, clip: CLIP, stop_at_clip_layer: int):
        clip = clip.clone()
        clip.clip_layer(stop_at_clip_layer)
        return (clip,)


class KSampler2:
    def sample(self, model, seed, steps, cfg, sampler_name, scheduler, positive, negative, latent_image, denoise=1.0,
               preview: Optional[LatentPreviewer] = None, apply_noise_mask: bool = False, apply_cond_areas: bool = False,
               apply_control: bool = False):
        """`preview`: a LatentPreviewer that shows the running latent through TAESD every step, where the reference's sampler loops call
        taesd_preview (LD.py:937, 1105, 1237); its `every` counts from this call's first step.  `apply_noise_mask`: honour
        latent_image["noise_mask"] (SetLatentNoiseMask) — redraw where it is 1, keep the latent where it is 0; off, the mask is not looked at, as in
        the reference.  `apply_cond_areas`: honour the conditioning entries' area, strength, mask and step range (ConditioningSetArea,
        ConditioningSetMask, ConditioningSetTimestepRange; sampling.sampling_function); off, those keys are inert, as in the reference.  `apply_control`: honour the
        entries' "control" key (ControlNetApply / ControlNetApplyAdvanced): the ControlNet's branch runs in every step inside its range; off, the
        key is inert, as in the reference."""
        if preview is not None:
            preview.reset()
        return common_ksampler(model, seed, steps, cfg, sampler_name, scheduler, positive, negative, latent_image, denoise=denoise, callback=preview,
                               apply_noise_mask=apply_noise_mask, apply_cond_areas=apply_cond_areas, apply_control=apply_control)


def _conditioning_set_values(conditioning, values: dict):
    """upstream's node_helpers.conditioning_set_values: a new list whose entries are [tensor, a copy of the dict with `values` set]"""
    out = []
    for t in conditioning:
        d = t[1].copy()
        d.update(values)
        out.append([t[0], d])
    return out


class ConditioningCombine:
    """combine(c1, c2) -> (c1 + c2,): both lists' entries in one list (upstream's node; the reference has none).  With apply_cond_areas every
    entry is weighed by its own area / mask / strength; without it the sampler averages them over the whole latent."""

    def combine(self, conditioning_1, conditioning_2):
        return (conditioning_1 + conditioning_2,)


class ConditioningSetArea:
    """append(conditioning, width, height, x, y, strength) -> (conditioning,): the entries apply to a rectangle given in PIXELS (// 8 = latent
    units), feathered over 8 latent pixels at its edges inside the latent (upstream's node)."""

    def append(self, conditioning, width, height, x, y, strength):
        return (_conditioning_set_values(conditioning, {"area": (height // 8, width // 8, y // 8, x // 8), "strength": strength,
                                                        "set_area_to_bounds": False}),)


class ConditioningSetAreaPercentage:
    """append(conditioning, width, height, x, y, strength): the rectangle as fractions of the latent (upstream's node)."""

    def append(self, conditioning, width, height, x, y, strength):
        return (_conditioning_set_values(conditioning, {"area": ("percentage", height, width, y, x), "strength": strength,
                                                        "set_area_to_bounds": False}),)


class ConditioningSetMask:
    """append(conditioning, mask, set_cond_area, strength): the entries are weighed by `mask` ([H, W] or [B, H, W], any resolution: resized to
    the latent) times `strength`; set_cond_area "mask bounds" also restricts the model call to the mask's bounding box (upstream's node)."""

    def append(self, conditioning, mask, set_cond_area, strength):
        if set_cond_area not in ("default", "mask bounds"):
            raise ValueError(f"set_cond_area must be 'default' or 'mask bounds', got {set_cond_area!r}")
        if len(mask.shape) < 3:
            mask = mask.unsqueeze(0)
        return (_conditioning_set_values(conditioning, {"mask": mask, "set_area_to_bounds": set_cond_area != "default", "mask_strength": strength}),)


class ConditioningSetTimestepRange:
    """set_range(conditioning, start, end): the entries are active from fraction `start` to fraction `end` of the schedule (upstream's node)."""

    def set_range(self, conditioning, start, end):
        return (_conditioning_set_values(conditioning, {"start_percent": start, "end_percent": end}),)


class ControlNetLoader:
    """load_controlnet(state_dict_or_path) -> (control_net,): a ControlNet in upstream's cldm key layout (time_embed.*, input_blocks.*,
    middle_block.*, input_hint_block.*, zero_convs.*, middle_block_out.*), with or without the `control_model.` prefix; the configuration is
    read from the shapes, as the checkpoint loader reads the UNet's.  Diffusers-layout files, T2I-Adapters and ControlLoRAs are refused
    (ValueError).  The workspace is sized on first use."""

    def __init__(self, device="cuda:0", unet_heads: int = 8, max_batch: int = 1, max_hw=(64, 64), max_tokens: int = 77):
        self.device, self.unet_heads, self.max_batch, self.max_hw, self.max_tokens = device, unet_heads, max_batch, max_hw, max_tokens

    def load_controlnet(self, control_net_name):
        from . import checkpoint as CK
        from .controlnet import ControlNet, MI355XControlNet
        sd = CK.load_state_dict(os.fspath(control_net_name)) if isinstance(control_net_name, (str, os.PathLike)) else dict(control_net_name)
        sd = CK.controlnet_state_dict(sd)
        cfg, hint_channels = CK.detect_controlnet_config(sd, num_heads=self.unet_heads)
        cm = MI355XControlNet(cfg, sd, hint_channels=hint_channels, device=self.device, max_batch=2 * self.max_batch, max_hw=self.max_hw,
                              max_tokens=self.max_tokens)
        return (ControlNet(cm),)


def load_synthetic_controlnet(device="cuda:0", max_batch: int = 1, max_hw=(64, 64), tiny: bool = False, seed: int = 0, max_tokens: int = 77,
                              hint_channels: int = 3):
    """A ControlNet with deterministic random-init weights on the synthetic UNet's configuration — the offline stand-in for a downloaded one.
    Its zero convolutions are NOT zero (weights.synth_controlnet_tensor): it visibly steers the synthetic UNet."""
    from .controlnet import ControlNet, synthetic_controlnet
    cfg = W.tiny_unet_config() if tiny else W.sd15_unet_config()
    return ControlNet(synthetic_controlnet(cfg, seed, hint_channels, device=device, max_batch=2 * max_batch, max_hw=max_hw, max_tokens=max_tokens))


class ControlNetApply:
    """apply_controlnet(conditioning, control_net, image, strength) -> (conditioning,) (upstream's node): every entry carries a copy of
    `control_net` with `image` ([B, H, W, 3] in [0, 1]) as its hint, and control_apply_to_uncond = True, so the sampler gives the negative list
    the same control.  KSampler2().sample(..., apply_control=True) honours it."""

    def apply_controlnet(self, conditioning, control_net, image, strength):
        if strength == 0:
            return (conditioning,)
        hint = image.movedim(-1, 1)
        c = []
        for t in conditioning:
            n = [t[0], t[1].copy()]
            cn = control_net.copy().set_cond_hint(hint, strength)
            if "control" in t[1]:
                cn.set_previous_controlnet(t[1]["control"])
            n[1]["control"] = cn
            n[1]["control_apply_to_uncond"] = True
            c.append(n)
        return (c,)


class ControlNetApplyAdvanced:
    """apply_controlnet(positive, negative, control_net, image, strength, start_percent, end_percent) -> (positive, negative) (upstream's node):
    both lists carry ONE copy of `control_net`, active from fraction start_percent to end_percent of the schedule; control_apply_to_uncond = False."""

    def apply_controlnet(self, positive, negative, control_net, image, strength, start_percent, end_percent):
        if strength == 0:
            return (positive, negative)
        hint = image.movedim(-1, 1)
        cnets = {}
        out = []
        for conditioning in (positive, negative):
            c = []
            for t in conditioning:
                d = t[1].copy()
                prev = d.get("control")
                if prev in cnets:
                    cn = cnets[prev]
                else:
                    cn = control_net.copy().set_cond_hint(hint, strength, (start_percent, end_percent))
                    cn.set_previous_controlnet(prev)
                    cnets[prev] = cn
                d["control"] = cn
                d["control_apply_to_uncond"] = False
                c.append([t[0], d])
            out.append(c)
        return (out[0], out[1])


class SetLatentNoiseMask:
    """set_mask(samples, mask) -> (latent,): a copy of the latent dict that carries `mask` (on the pixel grid or the latent grid, [H, W] or with
    leading axes; 1 = redraw, 0 = keep) as noise_mask [-1, 1, H, W].  Upstream's node; the reference has none because its sampler drops the mask.
    KSampler2().sample(..., apply_noise_mask=True) honours it (sampling.prepare_mask resizes it to the latent)."""

    def set_mask(self, samples, mask):
        s = samples.copy()
        s["noise_mask"] = mask.reshape((-1, 1, mask.shape[-2], mask.shape[-1]))
        return (s,)


class LoraLoader:
    """LoraLoader.load_lora (LD.py:6611-6625) = load_lora_for_models (LD.py:6203-6219): clones of the model and the clip that carry the
    LoRA as weight patches.  Nothing is merged here — the clones share the resident UNet / text model with their originals, and the patches
    are swapped into the resident weights on the device where a clone is next used (ModelPatcher.patch_model, CLIP.patch_model)."""

    def load_lora(self, model, clip, lora_name, strength_model, strength_clip):
        from . import checkpoint as CK
        lora = CK.load_state_dict(os.fspath(lora_name)) if isinstance(lora_name, (str, os.PathLike)) else lora_name
        new_model = model.clone() if model is not None else None
        new_clip = clip.clone() if clip is not None else None
        if strength_model == 0 and strength_clip == 0:
            return (new_model, new_clip)
        shapes = {}
        for part in (model, clip):
            if part is not None:
                shapes.update(part.model_key_shapes())
        keys = {k: torch.empty(s, device="meta") for k, s in shapes.items()}       # names and shapes only
        loaded = CK.resolve_lora(keys, lora, ModelPatcher.KEY_PREFIX, CLIP.KEY_PREFIX)
        loaded.warn()
        if new_model is not None and strength_model != 0:
            new_model.add_patches(loaded, strength_model)
        if new_clip is not None and strength_clip != 0:
            new_clip.add_patches(loaded, strength_clip)
        return (new_model, new_clip)


class VAEDecode:
    def decode(self, vae: MI355XVAE, samples):
        return (vae.decode(samples["samples"]),)


class VAEEncode:
    def encode(self, vae: MI355XVAE, pixels):
        return ({"samples": vae.encode(pixels[:, :, :, :3])},)


def bislerp(samples: torch.Tensor, width: int, height: int, device=None) -> torch.Tensor:
    """Latent upscale of the hires-fix path (bislerp, LD.py:429-518) on the HIP kernel `ld_op_bislerp`: a 2-tap separable
    resize along W then H whose blend of the two C-vectors slerps the direction and lerps the magnitude.  A host tensor
    (what KSampler2 returns, LD.py:3156-3203) is uploaded, resized on the device and returned to the host."""
    from . import ops
    if samples.is_cuda:
        return ops.bislerp(samples, width, height)
    # one rank per GPU: the default is THIS process's current device, never a hard-coded cuda:0
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    return ops.bislerp(samples.to(dev), width, height).to(samples.device)


class LatentUpscale:
    upscale_methods = ["nearest-exact", "bilinear", "area", "bicubic", "bislerp"]

    def __init__(self, device=None):
        self.device = device          # the model's load_device in a one-rank-per-GPU job (None: the current device)

    def upscale(self, samples, upscale_method, width, height, crop="disabled"):
        if width == 0 and height == 0:
            return (samples,)
        s = samples.copy()
        s["samples"] = bislerp(samples["samples"], max(64, width) // 8, max(64, height) // 8, device=self.device)   # the only mode (LD.py:521-523)
        return (s,)


class UpscaleModelLoader:
    """load_model(name) -> (upscale_model,) (LD.py:7240-7272): an RRDBNet state dict, or the name of one under `model_dir`, of any of
    the spellings checkpoint.normalize_esrgan_keys accepts."""

    def __init__(self, device="cuda:0", model_dir: Optional[str] = None):
        self.device, self.model_dir = device, model_dir

    def load_model(self, model_name):
        from . import checkpoint as CK
        if isinstance(model_name, str):
            path = model_name if os.path.isabs(model_name) or self.model_dir is None else os.path.join(self.model_dir, model_name)
            sd = torch.load(path, map_location="cpu", weights_only=True) if path.endswith((".pth", ".pt")) else CK.load_state_dict(path)
        else:
            sd = dict(model_name)
        cfg = CK.detect_esrgan_config(sd)
        return (MI355XUpscaler(cfg, CK.normalize_esrgan_keys(sd), device=self.device),)


class TAESDLoader:
    """load(name) -> (taesd,): the TAESD decoder of the latent preview from `taesd_decoder.safetensors` (LD.py:733-737), a path, a name
    under `model_dir`, or a state dict with Decoder2's keys."""

    def __init__(self, device="cuda:0", model_dir: Optional[str] = None):
        self.device, self.model_dir = device, model_dir

    def load(self, name="taesd_decoder.safetensors"):
        if isinstance(name, (str, os.PathLike)):
            name = os.fspath(name)
            name = name if os.path.isabs(name) or self.model_dir is None else os.path.join(self.model_dir, name)
        return (MI355XTAESD(name, device=self.device),)


class ImageUpscaleWithModel:
    """upscale(upscale_model, image) -> (image,) (LD.py:7356-7395): tiled_scale with tile 512 / overlap 32 (the reference's constants),
    clamped to [0, 1]; host fp32 [B, H, W, 3] in, host fp32 [B, H s, W s, 3] out.  Runs on the model's device."""

    def __init__(self, tile: int = 512, overlap: int = 32):
        self.tile, self.overlap = tile, overlap

    def upscale(self, upscale_model: MI355XUpscaler, image):
        s = tiled_upscale(upscale_model, image, self.tile, self.overlap)
        return (torch.clamp(s, min=0, max=1.0).cpu(),)


class UltimateSDUpscale:
    """upscale(...) -> (images,) (LD.py:8236-8324) with the reference's argument list: host fp32 [B, H, W, 3] in, host fp32
    [B, H', W', 3] out, H' = ceil(H upscale_by / 8) 8.  The upscale model, the tile-by-tile redraw and the Half Tile seam fix run on the
    device on a resident uint8 canvas (usdu.py; the 8-bit image kernels are bit-identical to the reference's Pillow plumbing).
    `stages`: replacement stage callables for the orchestration tests (usdu.upscale); the product path never passes it."""

    def upscale(self, image, model, positive, negative, vae, upscale_by, seed, steps, cfg, sampler_name, scheduler, denoise, upscale_model,
                mode_type, tile_width, tile_height, mask_blur, tile_padding, seam_fix_mode, seam_fix_denoise, seam_fix_mask_blur, seam_fix_width,
                seam_fix_padding, force_uniform_tiles, stages=None):
        from . import usdu
        return usdu.upscale(image, model, positive, negative, vae, upscale_by, seed, steps, cfg, sampler_name, scheduler, denoise, upscale_model,
                            mode_type, tile_width, tile_height, mask_blur, tile_padding, seam_fix_mode, seam_fix_denoise, seam_fix_mask_blur,
                            seam_fix_width, seam_fix_padding, force_uniform_tiles, stages=stages)


class SegsBitwiseAndMask:
    """doit(segs, mask) -> (segs,) (LD.py:8867-8869): every segment's mask AND the full-image mask, as bytes."""

    def doit(self, segs, mask):
        from . import detailer
        return (detailer.segs_bitwise_and_mask(segs, mask),)


class DetailerForEach:
    """doit(...) -> (image, cropped, cropped_enhanced, cropped_enhanced_alpha, cnet_pil_list) with the argument list of the reference's
    DetailerForEachTest.doit (LD.py:9598-9670): host fp32 [1, H, W, 3] in and out, the three lists of host fp32 crops sorted by shape, largest
    first, cnet_pil_list = [zeros(1, 64, 64, 3)] (empty_pil_tensor).  Every segment is redrawn on the model's device on a resident fp32 canvas
    (detailer.do_detail over the image kernels of lightdiffusion_amd.ops); `wildcard` is do_detail's wildcard_opt: "" or None."""

    def doit(self, image, segs, model, clip, vae, guide_size, guide_size_for, max_size, seed, steps, cfg, sampler_name, scheduler, positive, negative,
             denoise, feather, noise_mask, force_inpaint, wildcard, detailer_hook=None, cycle=1, inpaint_model=False, noise_mask_feather=0,
             scheduler_func_opt=None, apply_noise_mask=False, apply_cond_areas=False):
        """apply_noise_mask (not the reference's; off by default): the sampler honours the segment's noise mask, blurred by noise_mask_feather
        when that is > 0, and DifferentialDiffusion thresholds it per step (detailer.py, module docstring).  apply_cond_areas (likewise): every
        segment's sampler honours the conditioning entries' area / strength / mask / step range, on the segment's latent."""
        from . import detailer, ops
        if apply_noise_mask and noise_mask_feather > 0 and "denoise_mask_function" not in model.model_options:
            model = DifferentialDiffusion().apply(model)[0]          # what do_detail installs (LD.py:9451-9455), on the model the stages sample with
        stages = detailer.model_stages(model, vae, positive, negative, steps, cfg, sampler_name, scheduler, denoise, ops=ops,
                                       apply_noise_mask=apply_noise_mask, apply_cond_areas=apply_cond_areas)
        enhanced, cropped, cropped_enhanced, cropped_enhanced_alpha, _, _ = detailer.do_detail(
            image, segs, model, clip, vae, guide_size, guide_size_for, max_size, seed, steps, cfg, sampler_name, scheduler, positive, negative, denoise,
            feather, noise_mask, force_inpaint, wildcard, detailer_hook, cycle=cycle, inpaint_model=inpaint_model, noise_mask_feather=noise_mask_feather,
            scheduler_func_opt=scheduler_func_opt, stages=stages, apply_noise_mask=apply_noise_mask)
        return enhanced, cropped, cropped_enhanced, cropped_enhanced_alpha, [torch.zeros(1, 64, 64, 3)]


# ------------------------------------------------------------------ loaders
def load_synthetic_upscaler(device="cuda:0", nb: int = 23, scale: int = 4, seed: int = 0) -> MI355XUpscaler:
    """An RRDBNet with deterministic random-init weights: the offline stand-in for RealESRGAN_x4plus.pth (LD.py:84-90)."""
    return MI355XUpscaler(W.esrgan_config(nb, scale), lambda name, shape: W.synth_tensor(name, shape, seed), device=device)


def load_synthetic_taesd(device="cuda:0", seed: int = 0, **kw) -> MI355XTAESD:
    """A TAESD decoder with deterministic random-init weights: the offline stand-in for taesd_decoder.safetensors (LD.py:92-98)."""
    return MI355XTAESD(lambda name, shape: W.synth_tensor("taesd_decoder." + name, shape, seed), device=device, **kw)


def _attach(unet: MI355XUNet, device) -> ModelPatcher:
    patcher = ModelPatcher(SD15Model(unet), load_device=device)
    patcher.set_model_unet_function_wrapper(unet)
    return patcher


def load_synthetic(device="cuda:0", max_batch: int = 1, max_hw=(64, 64), tiny: bool = False, seed: int = 0, tokenizer_dir: Optional[str] = None,
                   max_tokens: int = 77, embedding_directory=None):
    """(model, clip, vae) with deterministic random-init weights — the offline stand-in for a downloaded checkpoint.
    `max_batch` / `max_hw` / `max_tokens` only pre-size the workspaces: larger batches, latents (hires pass) or prompts
    (more 77-token chunks) grow them on first use (MI355XUNet._ensure, MI355XVAE._ensure).  `embedding_directory`: where the tokenizer
    looks for the textual-inversion files that `embedding:name` words name (the reference's `_internal/embeddings/`)."""
    ucfg, vcfg, ccfg = (W.tiny_unet_config(), W.tiny_vae_config(), W.tiny_clip_config()) if tiny else \
        (W.sd15_unet_config(), W.sd15_vae_config(), W.sd15_clip_config())
    if tiny:
        ccfg = dict(ccfg, hidden_size=ucfg["context_dim"])
    gen = lambda name, shape: W.synth_tensor(name, shape, seed)
    unet = MI355XUNet(ucfg, gen, device=device, max_batch=2 * max_batch, max_hw=max_hw, max_tokens=max_tokens)
    vae = MI355XVAE(vcfg, gen, device=device, max_batch=max_batch, max_hw=max_hw, with_encoder=True)
    tok = PromptTokenizer.from_pretrained(tokenizer_dir, embedding_directory=embedding_directory,
                                          embedding_size=ccfg["hidden_size"]) if tokenizer_dir else None
    clip = CLIP(CLIPTextModelHIP(ccfg, W.synth_state_dict(W.clip_param_shapes(ccfg), seed), device=device), tok)
    return _attach(unet, device), clip, vae


class CheckpointLoaderSimple:
    """load_checkpoint(ckpt) -> (model, clip, vae) from a single-file SD1.x checkpoint (LD.py:6426-6513, 6591-6601): the
    architecture is detected from the keys (checkpoint.detect_*), weights are repacked on the device by the C library."""

    def __init__(self, device="cuda:0", max_batch: int = 1, max_hw=(64, 64), tokenizer_dir: Optional[str] = None,
                 clip_heads: int = 12, unet_heads: int = 8, max_tokens: int = 77, embedding_directory=None):
        self.device, self.max_batch, self.max_hw, self.tokenizer_dir = device, max_batch, max_hw, tokenizer_dir
        self.embedding_directory = embedding_directory      # textual-inversion files for `embedding:name` (SD1ClipModel's embedding_directory, LD.py:6598)
        self.clip_heads, self.unet_heads, self.max_tokens = clip_heads, unet_heads, max_tokens

    def load_checkpoint(self, ckpt_name, output_vae=True, output_clip=True, lora=None, lora_strength: float = 1.0,
                        lora_strength_clip: Optional[float] = None):
        """`lora`: a LoRA state dict or a path to one; merged into UNet AND text-encoder weights before they are uploaded
        (load_lora_for_models, LD.py:6203-6219: strength_model / strength_clip)."""
        from . import checkpoint as CK
        sd = CK.load_state_dict(ckpt_name) if isinstance(ckpt_name, str) else dict(ckpt_name)
        if lora is not None:
            CK.merge_lora(sd, CK.load_state_dict(lora) if isinstance(lora, str) else lora, lora_strength, lora_strength_clip)
        unet = MI355XUNet(CK.detect_unet_config(sd, num_heads=self.unet_heads), sd, device=self.device, max_batch=2 * self.max_batch,
                          max_hw=self.max_hw, max_tokens=self.max_tokens)
        vcfg, has_enc = CK.detect_vae_config(sd)
        vae = MI355XVAE(vcfg, sd, device=self.device, max_batch=self.max_batch, max_hw=self.max_hw, with_encoder=has_enc)
        csd = CK.clip_state_dict(sd)
        ccfg = CK.detect_clip_config(csd, self.clip_heads)
        tok = PromptTokenizer.from_pretrained(self.tokenizer_dir, embedding_directory=self.embedding_directory,
                                              embedding_size=ccfg["hidden_size"]) if self.tokenizer_dir else None
        clip = CLIP(CLIPTextModelHIP(ccfg, csd, device=self.device), tok)
        return _attach(unet, self.device), clip, vae


def _conditioning_of(clip, prompt):
    """a prompt string or pre-tokenised chunks through the text model -> [[cond, {"pooled_output": ..}]]; a conditioning list as it is"""
    if isinstance(prompt, (list, tuple)) and prompt and isinstance(prompt[0], (list, tuple)) and prompt[0] and isinstance(prompt[0][0], torch.Tensor):
        return list(prompt)
    cond, pooled = clip.encode_from_tokens(clip.tokenize(prompt) if isinstance(prompt, str) else prompt, return_pooled=True)
    return [[cond, {"pooled_output": pooled}]]


def txt2img(model, clip, vae, prompt_tokens, negative_tokens, width=512, height=512, batch_size=1, seed=0, steps=20, cfg=7.0,
            sampler_name="dpmpp_2m_sde", scheduler="karras", hires: bool = False, upscale_model: Optional[MI355XUpscaler] = None,
            preview: Optional[LatentPreviewer] = None, apply_cond_areas: bool = False, apply_control: bool = False):
    """The reference's headless `pipeline()` order (LD.py:10001-10086) with explicit arguments instead of hard-coded ones.
    `*_tokens`: a prompt string (needs a tokenizer on `clip`), pre-tokenised [[(id, weight), ...]] chunks, or a conditioning list
    [[tensor, {..}], ...] as the Conditioning* nodes build it.  `preview`: a LatentPreviewer for the first sampler pass (the hires pass has
    another latent shape and runs without one).  `apply_cond_areas`: both sampler passes honour the entries' area / strength / mask / step
    range (KSampler2).  `apply_control`: both passes honour the entries' ControlNet (the hint is resized and encoded again for the hires latent)."""
    pos, neg = _conditioning_of(clip, prompt_tokens), _conditioning_of(clip, negative_tokens)
    lat = EmptyLatentImage().generate(width, height, batch_size)[0]
    lat = KSampler2().sample(model, seed, steps, cfg, sampler_name, scheduler, pos, neg, lat, preview=preview, apply_cond_areas=apply_cond_areas,
                             apply_control=apply_control)[0]
    if hires:   # hires-fix (LD.py:10585-10603): bislerp x2, then 10 Euler-a steps at denoise 0.45, cfg 8
        lat = LatentUpscale(model.load_device).upscale(lat, "bislerp", width * 2, height * 2)[0]
        lat = KSampler2().sample(model, seed, 10, 8, "euler_ancestral", "normal", pos, neg, lat, denoise=0.45, apply_cond_areas=apply_cond_areas,
                                 apply_control=apply_control)[0]
    img = VAEDecode().decode(vae, lat)[0]
    if upscale_model is not None:   # the image-side upscale the reference builds next to the sampler nodes (LD.py:10014-10015)
        img = ImageUpscaleWithModel().upscale(upscale_model, img)[0]
    return img


def txt2img_sharded(model, clip, vae, prompt_tokens, negative_tokens, width=512, height=512, global_batch=8, seed=0, steps=20, cfg=7.0,
                    sampler_name="euler_ancestral", scheduler="normal", gather: bool = True, run_sampler=None):
    """Batched generation sharded over the ranks of one node (BASELINE config #4), in the call order of the
    reference's `pipeline()` (LD.py:10001-10086): rank 0 runs CLIP and broadcasts [cond, uncond] once (RCCL over xGMI;
    the only data-path collective), every rank takes a contiguous block of the global batch, draws the FULL-batch noise
    from the single seed on its host generator and keeps its rows (initial noise and every ancestral step), runs its own
    sampler loop on its own UNet replica and decodes its images; the images are gathered on rank 0 (None elsewhere).
    Row for row the result equals the single-process run of the same global batch.
    `run_sampler(noise, latent, pos, neg, sigmas, extra_options) -> latents` replaces the device sampler loop in the
    CPU (gloo) test of this host logic; the product path never passes it."""
    import torch.distributed as tdist
    from . import dist as D
    world = D.world_size()
    rank = tdist.get_rank() if world > 1 else 0
    enc = lambda t: clip.encode_from_tokens(clip.tokenize(t) if isinstance(t, str) else t, return_pooled=False)
    pc = nc = shapes = None
    if rank == 0:
        pc, nc = enc(prompt_tokens), enc(negative_tokens)
        shapes = [tuple(pc.shape), tuple(nc.shape)]
    if world > 1:
        box = [shapes]
        tdist.broadcast_object_list(box, src=0)                 # token counts (77 x chunks): a few bytes of metadata
        on_gpu = tdist.get_backend() == "nccl"
        pc, nc = D.broadcast_conditioning([pc, nc], box[0], src=0, device=None if on_gpu else torch.device("cpu"))
        pc, nc = pc.cpu(), nc.cpu()
    rows = D.shard_rows(global_batch, rank, world)
    b = rows.stop - rows.start
    lat_shape = (global_batch, 4, height // 8, width // 8)
    if b > 0:
        noise = D.full_batch_noise(lat_shape, seed, rows)
        latent = torch.zeros((b,) + lat_shape[1:])
        sigmas = sampling.calculate_sigmas(model.get_model_object("model_sampling"), scheduler, steps)
        dev = model.load_device
        extra = {}
        if sampler_name == "euler_ancestral":     # per-step noise: full-batch draw on the host generator, this rank's rows
            extra["noise_sampler"] = sampling.host_noise_sampler(torch.empty((b,) + lat_shape[1:], device=dev), rows, global_batch)
        pos, neg = [[pc, {"pooled_output": None}]], [[nc, {"pooled_output": None}]]
        if run_sampler is not None:
            samples = run_sampler(noise, latent, pos, neg, sigmas, extra)
        else:
            samples = sampling.sample(model, noise, pos, neg, cfg, dev, sampling.ksampler(sampler_name, extra), sigmas,
                                      model.model_options, latent_image=latent, seed=seed).cpu()
        images = vae.decode(samples)
    else:
        images = torch.zeros((0, height, width, 3))
    if not gather or world == 1:
        return images
    if tdist.get_backend() == "nccl":                          # 6.3 MB per rank as uint8
        g = D.gather_images((images * 255.0).round().to(torch.uint8).to(model.load_device), dst=0)
        return None if g is None else g.cpu().float() / 255.0
    return D.gather_images(images, dst=0)


def inpaint(model, clip, vae, image, mask, prompt_tokens, negative_tokens, seed=0, steps=20, cfg=7.0, sampler_name="dpmpp_2m_sde", scheduler="karras",
            denoise=1.0, apply_cond_areas: bool = False, apply_control: bool = False):
    """Masked redraw of an image: VAEEncode, SetLatentNoiseMask, KSampler2(apply_noise_mask=True), VAEDecode.  image: host fp32 [B, H, W, 3] in
    [0, 1], H and W multiples of 64; mask [H, W] or [B, H, W] (or the latent grid's), 1 where the image is redrawn and 0 where its latent is kept
    -> host fp32 [B, H, W, 3].  `*_tokens`, `apply_cond_areas` and `apply_control` as in txt2img.  The kept region goes through the VAE and back; nothing is
    composited in pixel space."""
    pos, neg = _conditioning_of(clip, prompt_tokens), _conditioning_of(clip, negative_tokens)
    lat = VAEEncode().encode(vae, image)[0]
    lat = SetLatentNoiseMask().set_mask(lat, torch.as_tensor(mask, dtype=torch.float32))[0]
    lat = KSampler2().sample(model, seed, steps, cfg, sampler_name, scheduler, pos, neg, lat, denoise=denoise, apply_noise_mask=True,
                             apply_cond_areas=apply_cond_areas, apply_control=apply_control)[0]
    return VAEDecode().decode(vae, lat)[0]


def img2img(model, clip, vae, upscale_model, image, prompt_tokens, negative_tokens, upscale_by=2, seed=0, steps=8, cfg=6, sampler_name="dpmpp_2m_sde",
            scheduler="karras", denoise=0.3, mode_type="Linear", tile_width=512, tile_height=512, mask_blur=16, tile_padding=32,
            seam_fix_mode="Half Tile", seam_fix_denoise=0.2, seam_fix_mask_blur=16, seam_fix_width=64, seam_fix_padding=32,
            force_uniform_tiles="enable"):
    """The reference's img2img (`_img2img`, LD.py:10325-10417) in its call order, its constants as defaults: both prompts through the text
    model, then UltimateSDUpscale on the image [B, H, W, 3] (host fp32 in [0, 1]) -> host fp32 [B, H', W', 3].  `*_tokens` as in txt2img.
    (The reference sets CLIP's last layer to -2 and loads a LoRA first: CLIPSetLastLayer / LoraLoader on `clip` / `model` before the call.)"""
    enc = lambda t: clip.encode_from_tokens(clip.tokenize(t) if isinstance(t, str) else t, return_pooled=True)
    (pc, pp), (nc, npool) = enc(prompt_tokens), enc(negative_tokens)
    pos, neg = [[pc, {"pooled_output": pp}]], [[nc, {"pooled_output": npool}]]
    return UltimateSDUpscale().upscale(image, model, pos, neg, vae, upscale_by, seed, steps, cfg, sampler_name, scheduler, denoise, upscale_model,
                                       mode_type, tile_width, tile_height, mask_blur, tile_padding, seam_fix_mode, seam_fix_denoise, seam_fix_mask_blur,
                                       seam_fix_width, seam_fix_padding, force_uniform_tiles)[0]
