"""The Detailer (DetailerForEach.do_detail, LD.py:9402-9590; enhance_detail, LD.py:9208-9352): every segment of `segs` is cropped from the
CURRENT image, Lanczos-resized to a work size, VAE-encoded, denoised for a few steps, VAE-decoded, Lanczos-resized back and pasted over
the crop through the segment's feathered mask.  The detectors that make the segments in the reference (YOLO, SAM, cv2) are third-party
networks and stay outside this package; `segs_from_boxes` builds what the box detector builds from boxes the caller has.

The reference does the image plumbing on the host, with numpy, PIL and torchvision, for every segment.  The loop here (`do_detail`) is
written for a canvas that goes up once as fp32 [H, W, 3] and comes down once, over an op namespace it is handed: the Pillow-identical
`u8_resample` / `u8_from_f32` / `f32_from_u8` of lightdiffusion_amd.ops, and three fp32 image ops — `u8_crop_from_f32` (tensor2pil of a window
of the canvas), `f32_gaussian_blur` (the mask blur) and `f32_paste_u8_` (pil2tensor + tensor_paste), HIP kernels too (csrc/detail/detail_image.hip:
crop and paste bit-identical to the reference's fp32 arithmetic, the blur within a derived bound of torchvision's).  `model_stages` builds the
encode / sample / decode stages on the resident VAE and sampler for such a namespace, and nodes.DetailerForEach hands `do_detail` the stages
over lightdiffusion_amd.ops: the device Detailer.  `do_detail` itself takes its `stages` from the caller and raises without — the tests run it
on a NumPy namespace as well — and nothing here falls back to torch on the host.  Only the small latents cross to the host, as in usdu.py.
This module holds the geometry (pure Python / NumPy) and the segment loop; it imports neither PIL nor torchvision.

THE ONE DEVIATION: the work size.  The reference encodes and denoises at (new_w, new_h) = int(side * upscale) whatever they are; its UNet
resizes to the skip's shape on the way up.  The UNet here takes latent sides that are multiples of 8 only, so the crop is Lanczos-resized to
(W64, H64): new_w and new_h each rounded UP to a multiple of 64 and capped at max(64, max_size // 64 * 64); the decoded (W64, H64) image is
Lanczos-resized back to the crop's (w, h).  Where the reference's size is a multiple of 64 already the flow is the reference's step for step
(the goldens pin that case); otherwise the crop is stretched by at most 63 px a side and un-stretched on the way back.  See `work_size`.

Behaviours of the reference that are mirrored on purpose:
  * the crop comes from the current image, never from seg.cropped_image, so overlapping segments see earlier pastes (LD.py:9458-9461);
  * the paste alpha is tensor_gaussian_blur_mask(seg.cropped_mask, feather) (LD.py:8979-9004): torchvision's GaussianBlur(2 feather + 1,
    sigma = 10) on the fp32 mask, reflect padding;
  * a segment whose mask is all zero is skipped AFTER its index is taken: the segment seed is seed + i over all segments (LD.py:9465-9474);
  * THE SAMPLER-LEVEL NOISE MASK IS INERT.  enhance_detail blurs the mask a second time (noise_mask_feather) and hands it to the sampler
    as latent["noise_mask"], but KSamplerX0Inpaint.__call__ (LD.py:2629-2636) receives denoise_mask and ignores it, so
    DifferentialDiffusion.forward (LD.py:8951-8965), which do_detail installs when noise_mask_feather > 0 (LD.py:9451-9455), is never
    called and that blur feeds nothing.  The images of the reference are mirrored: the mask reaches the paste and nothing else.  The
    second blur is not computed; the model is still cloned and given the function, and the un-blurred mask rides along as
    latent["noise_mask"] into sampling.sample's denoise_mask, where it is as inert as there.
    WITH apply_noise_mask=True (model_stages, do_detail, nodes.DetailerForEach; off by default, and nothing above changes while it is off) the
    mask is honoured: the second blur is computed on the device (ops.f32_gaussian_blur(mask, noise_mask_feather, 10), when noise_mask_feather > 0),
    that mask is the latent's noise_mask, the stage's sampler applies it (sampling.KSamplerX0Inpaint: two fp32 blend kernels around the model
    call) and DifferentialDiffusion.forward is called once per model call.  The redraw is then held to the crop's latent where the mask is 0,
    in the sampler and not only by the final paste.  These images are no longer the reference's, which cannot make them;
  * torchvision's GaussianBlur draws its sigma with torch.empty(1).uniform_(10, 10) on the host's global generator in every call, which moves
    the stream the VAE's posterior sample is drawn from next.  The draws are repeated here in the reference's places (one per segment before
    the empty-mask test, one per detailed segment for the inert noise-mask blur), so that a seeded run consumes the generator as it does;
  * guide_size_for_bbox, noise_mask (the flag) and force_inpaint are accepted and unused, as in the reference: the crop is always measured by
    its own size, and "force inpaint" is what happens whenever upscale <= 1;
  * THE BATCH IS 1: tensor2pil squeezes dim 0 (LD.py:8505-8509) and TensorBatchBuilder.concat keeps the last image only (LD.py:8880-8885),
    so a batch would come out as its last image pasted over the first.  B != 1 is a ValueError.
Also a ValueError where the reference misbehaves silently or crashes: segs[0] that is not the image's (H, W) (segs_scale_match returns None
there, LD.py:8912-8920), feather >= the crop's smaller side (torch's reflect pad refuses it), and every argument that is out of scope when it
is not at the reference's default (wildcard_opt, detailer_hook, the refiner arguments, inpaint_model, scheduler_func_opt, a segment's
control_net_wrapper, a conditioning mask).
"""
from __future__ import annotations

import math
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import torch

SEG = namedtuple("SEG", ["cropped_image", "cropped_mask", "confidence", "crop_region", "bbox", "label", "control_net_wrapper"], defaults=[None])
BLUR_SIGMA = 10.0          # tensor_gaussian_blur_mask's default, never overridden by the reference


# ------------------------------------------------------------------ geometry (pure Python)
def normalize_region(limit, startp, size):
    """LD.py:8539-8550: the interval [startp, startp + size) moved into [0, limit) and clipped to it -> (start, end) as ints."""
    if startp < 0:
        start, end = 0, min(limit, size)
    elif startp + size > limit:
        start, end = max(0, limit - size), limit
    else:
        start, end = startp, min(limit, startp + size)
    return int(start), int(end)


def make_crop_region(w, h, bbox, crop_factor, crop_min_size=None):
    """LD.py:8553-8575: the bbox (x1, y1, x2, y2) grown by crop_factor about its centre, moved into the w x h image -> [x1, y1, x2, y2]."""
    bw, bh = bbox[2] - bbox[0], bbox[3] - bbox[1]
    cw, ch = bw * crop_factor, bh * crop_factor
    x1 = int(bbox[0] + bw / 2 - cw / 2)
    y1 = int(bbox[1] + bh / 2 - ch / 2)
    x1, x2 = normalize_region(w, x1, cw)
    y1, y2 = normalize_region(h, y1, ch)
    return [x1, y1, x2, y2]


def work_size(w, h, guide_size, max_size):
    """-> (new_w, new_h, W64, H64) for a w x h crop.  (new_w, new_h) is enhance_detail's size (LD.py:9252-9267): the smaller side scaled
    to guide_size, both rescaled when one exceeds max_size, the crop's own size when that is no enlargement ("force inpaint").  (W64, H64)
    is the size this port works at: each rounded up to a multiple of 64, capped at max(64, max_size // 64 * 64) (module docstring)."""
    upscale = guide_size / min(w, h)
    new_w, new_h = int(w * upscale), int(h * upscale)
    if new_w > max_size or new_h > max_size:
        upscale *= max_size / max(new_w, new_h)
        new_w, new_h = int(w * upscale), int(h * upscale)
    if upscale <= 1.0 or new_w == 0 or new_h == 0:
        new_w, new_h = w, h
    cap = max(64, max_size // 64 * 64)
    up64 = lambda v: min(-(-v // 64) * 64, cap)
    return new_w, new_h, up64(new_w), up64(new_h)


def detail_sigmas(model_sampling, scheduler, steps, denoise):
    """ksampler_wrapper + separated_sample (LD.py:9113-9205): the last `steps` intervals of a floor(steps / denoise)-step schedule."""
    from .sampling import calculate_sigmas
    advanced = math.floor(steps / denoise)
    return calculate_sigmas(model_sampling, scheduler, advanced)[advanced - steps:]


def segs_from_boxes(image, boxes, masks=None, crop_factor=2.0, drop_size=10, confidences=None, labels=None):
    """What UltraBBoxDetector.detect (LD.py:8628-8673) builds from its detections, for boxes the caller has: image [1, H, W, C], boxes
    (x0, y0, x1, y1) in pixels -> segs = ((H, W), [SEG...]) in box order; a box is kept when both its sides exceed max(drop_size, 1).
    masks[i]: a full-image [H, W] mask (taken as fp32); by default the filled rectangle [int(x0)..int(x1)] x [int(y0)..int(y1)], both ends
    included, as cv2.rectangle(..., -1) draws it (inference_bbox, LD.py:8484-8489).  The detector's cv2.dilate (dilation) is not applied:
    pass dilated masks."""
    H, W = int(image.shape[1]), int(image.shape[2])
    drop = max(drop_size, 1)
    items = []
    for i, box in enumerate(boxes):
        box = np.asarray(box, dtype=np.float32)
        x0, y0, x1, y1 = box
        if masks is not None:
            mask = np.asarray(masks[i], dtype=np.float32)
            if mask.shape != (H, W):
                raise ValueError(f"masks[{i}] has shape {mask.shape}, expected the image's {(H, W)}")
        else:
            mask = np.zeros((H, W), np.float32)
            mask[max(int(y0), 0):max(int(y1) + 1, 0), max(int(x0), 0):max(int(x1) + 1, 0)] = 1.0
        if not (x1 - x0 > drop and y1 - y0 > drop):
            continue
        region = make_crop_region(W, H, box, crop_factor)
        items.append(SEG(image[:, region[1]:region[3], region[0]:region[2], :], mask[region[1]:region[3], region[0]:region[2]],
                         np.float32(1.0) if confidences is None else confidences[i], region, box, "" if labels is None else labels[i], None))
    return (H, W), items


def segs_bitwise_and_mask(segs, mask):
    """LD.py:8836-8864: every segment's mask AND the full-image mask inside its crop region — both as uint8(255 m), a bitwise & of the
    bytes (not a product: 0.5 & 1.0 is 127 & 255), back to fp32 / 255.  The control_net_wrapper is dropped, as there."""
    mask = torch.as_tensor(mask)
    while mask.dim() > 2:                     # make_2d_mask (LD.py:8732-8737)
        mask = mask.squeeze(0)
    full = (mask.cpu().numpy() * 255).astype(np.uint8)
    items = []
    for seg in segs[1]:
        x1, y1, x2, y2 = seg.crop_region
        both = np.bitwise_and((seg.cropped_mask * 255).astype(np.uint8), full[y1:y2, x1:x2])
        items.append(SEG(seg.cropped_image, both.astype(np.float32) / 255.0, seg.confidence, seg.crop_region, seg.bbox, seg.label, None))
    return segs[0], items


class DifferentialDiffusion:
    """LD.py:8945-8965.  `apply` gives a clone of the model whose model_options carry `forward` as the denoise-mask function; `forward`
    thresholds the mask by how far the current timestep is through the run.  Nothing in the reference's sampler calls it (module
    docstring): it is here because do_detail installs it and user code may."""

    def apply(self, model):
        model = model.clone()
        model.set_model_denoise_mask_function(self.forward)
        return (model,)

    def forward(self, sigma: torch.Tensor, denoise_mask: torch.Tensor, extra_options: dict):
        ms = extra_options["model"].inner_model.model_sampling
        if sigma.is_cuda:
            # the masked sampler step (sampling.KSamplerX0Inpaint) calls this once per model call with the step's sigma on the device: the same
            # threshold and comparison there, so that no step waits for the host to read sigma.  The run's two constant timesteps come from host
            # values and are looked up once per run (the run's `sigmas` tensor is one object from its first step to its last)
            sigmas = extra_options["sigmas"]
            run = self.__dict__.get("_run")
            if run is None or run[0] is not sigmas or run[1] is not ms:
                run = self._run = (sigmas, ms, int(ms.timestep(sigmas[0])), int(ms.timestep(ms.sigma_min)))
            _, _, ts_from, ts_to = run
            threshold = (ms.timestep_on_device(sigma[0]) - ts_to) / (ts_from - ts_to)
            return (denoise_mask >= threshold).to(denoise_mask.dtype)
        ts_from, ts_to = ms.timestep(extra_options["sigmas"][0]), ms.timestep(ms.sigma_min)
        threshold = (ms.timestep(sigma[0]) - ts_to) / (ts_from - ts_to)
        return (denoise_mask >= threshold).to(denoise_mask.dtype)


# ------------------------------------------------------------------ the run
def model_stages(model, vae, positive, negative, steps, cfg, sampler_name, scheduler, denoise, ops, apply_noise_mask=False, apply_cond_areas=False):
    """Stages on the resident VAE and sampler, for the op namespace `ops` (module docstring).  Pixels stay on the model's device; latents go
    through the host (the posterior sample and the sampler's noise are drawn on the host generator, as the reference does: VAE.encode's randn
    first, then prepare_noise's manual_seed(seed)).  sample(latent, seed) is ksampler_wrapper (LD.py:9160-9205): the tail of the longer
    schedule, noise added; the latent's noise_mask goes to sampling.sample's denoise_mask, inert there as in the reference — unless
    apply_noise_mask: then the sampler honours it (module docstring), with the denoise-mask function of `model`, where it has one.
    apply_cond_areas: the sampler honours the conditioning entries' area / strength / mask / step range on the segment's latent
    (sampling.sampling_function); off, they are inert as in the reference."""
    from . import sampling
    inpaint_options = {"apply_denoise_mask": True} if apply_noise_mask else None
    cond_areas = {"apply_cond_areas": True} if apply_cond_areas else {}      # (off: the call is the one it has always been)

    def sample(latent, seed):
        x = latent["samples"]
        noise = sampling.prepare_noise(x, seed)
        sigmas = detail_sigmas(model.get_model_object("model_sampling"), scheduler, steps, denoise)
        sampler = sampling.ksampler(sampler_name, inpaint_options=inpaint_options)
        out = sampling.sample(model, noise, positive, negative, cfg, model.load_device, sampler, sigmas, model.model_options,
                              latent_image=x, denoise_mask=latent.get("noise_mask"), seed=seed, **cond_areas)
        return dict(latent, samples=out.to("cpu"))

    return SimpleNamespace(ops=ops, device=torch.device(model.load_device), observe=None,
                           encode=lambda px: {"samples": vae.encode(px)}, sample=sample, decode=lambda lat: vae.decode_device(lat["samples"]))


def _refuse_out_of_scope(positive, negative, **given):
    for name, (value, ok) in given.items():
        if not ok:
            raise ValueError(f"{name}={value!r} is not supported by this Detailer (wildcards, hooks, the refiner, inpaint models and "
                             f"scheduler functions are out of scope): leave {name} at the reference's default")
    for name, conds in (("positive", positive), ("negative", negative)):
        for c in conds or []:
            if isinstance(c[1], dict) and "mask" in c[1]:
                raise ValueError(f"{name}: a conditioning with a 'mask' would be cropped per segment by the reference; that is not supported")


def do_detail(image, segs, model, clip, vae, guide_size, guide_size_for_bbox, max_size, seed, steps, cfg, sampler_name, scheduler, positive, negative,
              denoise, feather, noise_mask, force_inpaint, wildcard_opt=None, detailer_hook=None, refiner_ratio=None, refiner_model=None,
              refiner_clip=None, refiner_positive=None, refiner_negative=None, cycle=1, inpaint_model=False, noise_mask_feather=0,
              scheduler_func_opt=None, stages=None, apply_noise_mask=False):
    """DetailerForEach.do_detail (LD.py:9402-9590) with the reference's argument list: image [1, H, W, 3] fp32 in [0, 1], segs = ((H, W),
    [SEG...]) -> (image, cropped_list, enhanced_list, enhanced_alpha_list, cnet_pil_list, (segs[0], new_segs)), host fp32 tensors; the
    lists are sorted by shape, largest first, as there; enhanced_alpha is the enhanced crop with the blurred mask as a fourth channel;
    cnet_pil_list is empty.  See the module docstring for the work size, the inert noise mask and the other mirrored behaviours.
    `stages` (required): a namespace of stage callables and image ops — encode(pixels [1, h, w, 3]) -> latent dict, sample(latent, seed),
    decode(latent) -> [1, h, w, 3], ops, device, observe (or None, called after every paste).  Every detailed segment's crop, enhanced crop
    and alpha stay on `device` until the one download at the end: memory grows with the number of segments, each of crop size.
    apply_noise_mask (not the reference's; off by default): with noise_mask_feather > 0 the second blur is computed and is the latent's noise_mask,
    for stages whose sampler honours it (model_stages(..., apply_noise_mask=True) on a model that carries the denoise-mask function)."""
    if stages is None:
        raise ValueError("do_detail needs `stages` (model_stages(..., ops=lightdiffusion_amd.ops) for the device; nodes.DetailerForEach builds "
                         "them): there is no fall-back to the host (see the module docstring)")
    if image.dim() != 4 or image.shape[-1] != 3:
        raise ValueError(f"expected an image [1, H, W, 3], got {tuple(image.shape)}")
    if image.shape[0] != 1:
        raise ValueError(f"a batch of {image.shape[0]} images: the reference's Detailer works on one image (tensor2pil squeezes the batch axis and "
                         f"TensorBatchBuilder.concat keeps the last image only, so a batch would be returned as its last crop); pass images one by one")
    H, W = int(image.shape[1]), int(image.shape[2])
    if not (tuple(segs[0]) == (H, W) or segs[0][0] == 0 or segs[0][1] == 0):
        raise ValueError(f"segs were made for a {tuple(segs[0])} image, this one is {(H, W)}: the reference's segs_scale_match returns None there")
    _refuse_out_of_scope(positive, negative, wildcard_opt=(wildcard_opt, wildcard_opt in (None, "")), detailer_hook=(detailer_hook, detailer_hook is None),
                         refiner_ratio=(refiner_ratio, refiner_ratio is None), refiner_model=(refiner_model, refiner_model is None),
                         refiner_clip=(refiner_clip, refiner_clip is None), refiner_positive=(refiner_positive, refiner_positive is None),
                         refiner_negative=(refiner_negative, refiner_negative is None), inpaint_model=(inpaint_model, inpaint_model is False),
                         scheduler_func_opt=(scheduler_func_opt, scheduler_func_opt is None))
    cycle, feather = int(cycle), int(feather)
    if cycle < 1:
        raise ValueError(f"cycle={cycle}: at least one sampler pass per segment")
    if feather < 0:
        raise ValueError(f"feather={feather} must not be negative")
    for i, seg in enumerate(segs[1]):
        x1, y1, x2, y2 = seg.crop_region
        if not (0 <= x1 < x2 <= W and 0 <= y1 < y2 <= H):
            raise ValueError(f"segment {i}: crop region {list(seg.crop_region)} does not lie inside the {W} x {H} image")
        if tuple(np.shape(seg.cropped_mask)) != (y2 - y1, x2 - x1):
            raise ValueError(f"segment {i}: mask of shape {tuple(np.shape(seg.cropped_mask))} for a crop of {(y2 - y1, x2 - x1)}")
        if feather >= min(y2 - y1, x2 - x1):
            raise ValueError(f"segment {i}: feather={feather} needs a crop larger than that on both sides, this one is {x2 - x1} x {y2 - y1} "
                             f"(the blur pads by reflection)")
        if seg.control_net_wrapper is not None:
            raise ValueError(f"segment {i}: control_net_wrapper is not supported (ControlNet is out of scope)")

    if model is not None and noise_mask_feather > 0 and "denoise_mask_function" not in model.model_options:
        model = DifferentialDiffusion().apply(model)[0]                                  # LD.py:9451-9455; inert: the stages sample with THEIR model
    st = stages
    ops, dev = st.ops, st.device
    sigma_draw = lambda: torch.empty(1).uniform_(BLUR_SIGMA, BLUR_SIGMA)                 # torchvision's GaussianBlur.get_params, for the generator only

    canvas = image[0].detach().to(dev, torch.float32, copy=True).contiguous()            # the one upload
    kept = []                                                                            # per detailed segment, on the device until the end
    for i, seg in enumerate(segs[1]):
        x1, y1, x2, y2 = (int(v) for v in seg.crop_region)
        w, h = x2 - x1, y2 - y1
        mask = np.ascontiguousarray(seg.cropped_mask, dtype=np.float32)
        sigma_draw()
        if not mask.any():                                                               # skipped, but i has advanced (LD.py:9465-9468)
            continue
        alpha = ops.f32_gaussian_blur(torch.from_numpy(mask).to(dev), feather, BLUR_SIGMA)
        seg_seed = seed + i
        new_w, new_h, W64, H64 = work_size(w, h, guide_size, max_size)
        sigma_draw()                                                                     # the noise-mask blur of enhance_detail: drawn, computed below if asked for
        crop_u8 = ops.u8_crop_from_f32(canvas, x1, y1, x2, y2)
        original = canvas[y1:y2, x1:x2].clone()
        tile = ops.u8_resample(crop_u8, (W64, H64), "lanczos")
        latent = st.encode(ops.f32_from_u8(tile)[None])
        if apply_noise_mask and noise_mask_feather > 0:
            latent["noise_mask"] = ops.f32_gaussian_blur(torch.from_numpy(mask).to(dev), int(noise_mask_feather), BLUR_SIGMA)[None]
        else:
            latent["noise_mask"] = torch.from_numpy(mask)[None]
        for c in range(cycle):                                                           # the same latent again, at seed + c (LD.py:9286-9330)
            latent = st.sample(latent, seg_seed + c)
        decoded = st.decode(latent).to(dev, torch.float32)
        back = ops.u8_resample(ops.u8_from_f32(decoded)[0], (w, h), "lanczos")
        ops.f32_paste_u8_(canvas, back, alpha, x1, y1)
        kept.append((seg, original, ops.f32_from_u8(back), alpha))
        if st.observe is not None:
            st.observe(SimpleNamespace(index=i, seed=seg_seed, crop=(x1, y1, x2, y2), size=(new_w, new_h), work_size=(W64, H64), alpha=alpha, tile=tile,
                                       canvas=canvas))

    out = canvas.cpu()[None]                                                             # the one download (and the segments' crops with it)
    cropped_list, enhanced_list, alpha_list, new_segs = [], [], [], []
    for seg, original, enhanced, alpha in kept:
        enhanced = enhanced.cpu()[None]
        cropped_list.append(original.cpu()[None])
        enhanced_list.append(enhanced)
        alpha_list.append(torch.cat((enhanced, alpha.cpu()[None, :, :, None]), dim=-1))
        new_segs.append(SEG(enhanced.numpy(), seg.cropped_mask, seg.confidence, seg.crop_region, seg.bbox, seg.label, seg.control_net_wrapper))
    for lst in (cropped_list, enhanced_list, alpha_list):
        lst.sort(key=lambda t: tuple(t.shape), reverse=True)
    return out, cropped_list, enhanced_list, alpha_list, [], (segs[0], new_segs)
