"""Live latent preview on one MI355X: TAESD's decoder (TAESD.decode on Decoder2, LD.py:688-754) behind the sampler loops' per-step callback,
where the reference calls `taesd_preview` (LD.py:761-768; LD.py:937, 1105, 1237).

`MI355XTAESD` owns an `ld_taesd` handle (31 convolutions on HIP kernels, csrc/taesd.hip); `LatentPreviewer` is the sampler `callback` that
decodes the running latent, copies the uint8 image to the host and hands it to the caller's `on_image`.

The picture: the reference pins `TAESD.decode` (range [-1, 1]); its `taesd_preview` then multiplies by 255 and loops over the three channel
PLANES, so that what it shows is the last plane as a grey image.  That loop's artefact is not reproduced: the image here is RGB through the
`(d + 1) / 2` map that `VAE.decode` uses (LD.py:6380), as `uint8(clip(255 ((d + 1) * 0.5), 0, 255))`.
"""
from __future__ import annotations

import os
from typing import Callable, Dict, Optional, Union

import torch

from . import weights as W
from ._lib import check, lib
from ._model import ResidentModel, WeightSource, _stream

_PREFIX = "taesd_decoder."


def decoder_state_dict(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """Any spelling of the decoder's state dict -> Decoder2's own keys (`1.weight` .. `19.bias`): `taesd_decoder.safetensors` has them bare; a
    whole TAESD module's state dict carries them under `taesd_decoder.` next to the encoder and the two scalars `vae_shift` /
    `vae_scale`, which are the constants 0 and 1 (LD.py:729-730) and are dropped."""
    want = W.taesd_decoder_param_shapes()
    out = {}
    for k, v in sd.items():
        for p in ("", _PREFIX):
            if k.startswith(p) and k[len(p):] in want:
                out[k[len(p):]] = v
                break
    missing = [k for k in want if k not in out]
    if missing:
        raise KeyError(f"not a TAESD decoder state dict: missing {missing[:4]}{' ...' if len(missing) > 4 else ''}")
    return out


def load_decoder_file(path: str) -> Dict[str, torch.Tensor]:
    from . import checkpoint as CK
    return decoder_state_dict(CK.load_state_dict(os.fspath(path)))


class MI355XTAESD(ResidentModel):
    """TAESD's decoder resident on one MI355X.  `weights`: a state dict (any spelling `decoder_state_dict` accepts), a callable
    (name, shape) -> tensor, or the path of a safetensors file.  The latent is what the sampler loop holds: the model-space x the reference
    passes to `taesd_preview` (LD.py:764), [B, 4, h, w], with no `process_out` applied."""

    family = "taesd"

    def __init__(self, weights: Union[WeightSource, str, os.PathLike], device="cuda:0", max_batch: int = 1, max_hw=(64, 64)):
        self.device = torch.device(device)
        if isinstance(weights, (str, os.PathLike)):
            weights = load_decoder_file(weights)
        elif not callable(weights):
            weights = decoder_state_dict(weights)
        self._create(weights)
        self._ensure(max_batch, max_hw[0], max_hw[1])

    def _nhwc(self, latent: torch.Tensor) -> torch.Tensor:
        if latent.dim() != 4 or latent.shape[1] != 4:
            raise ValueError(f"expected a latent batch [B, 4, h, w], got {tuple(latent.shape)}")
        return latent.to(self.device, torch.float32).permute(0, 2, 3, 1).contiguous()

    def decode_into(self, latent_nhwc: torch.Tensor, out: torch.Tensor, image: Optional[torch.Tensor] = None, profile: bool = False) -> None:
        """The enqueue alone, on caller-owned device buffers: latent_nhwc [B, h, w, 4] fp32 -> out [B, 8h, 8w, 3] fp32 and, when given,
        image [B, 8h, 8w, 3] uint8.  Allocates nothing once the workspace covers the shape: what a captured graph replays."""
        b, h, w, _ = latent_nhwc.shape
        self._ensure(b, h, w)
        fn, name = (lib().ld_taesd_profile, "ld_taesd_profile") if profile else (lib().ld_taesd_decode, "ld_taesd_decode")
        with torch.cuda.device(self.device):
            check(fn(self._h, latent_nhwc.data_ptr(), out.data_ptr(), None if image is None else image.data_ptr(), b, h, w, _stream()), name)

    def _run(self, latent: torch.Tensor, want_image: bool, profile: bool = False):
        x = self._nhwc(latent)
        b, h, w, _ = x.shape
        out = torch.empty(b, 8 * h, 8 * w, 3, dtype=torch.float32, device=self.device)
        img = torch.empty(b, 8 * h, 8 * w, 3, dtype=torch.uint8, device=self.device) if want_image else None
        self.decode_into(x, out, img, profile)
        return out, img

    def decode(self, latent: torch.Tensor) -> torch.Tensor:
        """[B, 4, h, w] -> TAESD.decode's [-1, 1]-ranged output as NHWC [B, 8h, 8w, 3] fp32 on the device."""
        return self._run(latent, False)[0]

    def image(self, latent: torch.Tensor) -> torch.Tensor:
        """[B, 4, h, w] -> the preview image [B, 8h, 8w, 3] uint8 on the device."""
        return self._run(latent, True)[1]

    def profile(self, latent: torch.Tensor) -> list:
        """One decode with HIP events around every launch -> [(what, dims, flops, microseconds, kernel)] in launch order."""
        self._run(latent, True, profile=True)
        return self.profile_launches()

    def to(self, device):
        """The reference builds a TAESD per preview and leaves it where it loads; the weights here stay resident in the C handle."""
        return self


class LatentPreviewer:
    """A sampler `callback` ({"x", "i", "sigma", "denoised"}) that shows the running latent through TAESD.

    On every `every`-th call since construction / `reset()` it decodes `rows` (default: image 0, like the reference) of `x` — or, with
    source="denoised", of `denoised`, falling back to `x` where the sampler has none (dpm_adaptive) —, copies the uint8 image into a pinned
    host buffer on the current stream, waits on THAT copy's event only, and calls `on_image(i, image)` with a uint8 [rows, H, W, 3] CPU
    tensor of its own.  Delivery is synchronous and uses no threads: the reference's fire-and-forget thread races with the loop.  The
    previewer only reads the latent, so the trajectory is the one without a preview.

    use_graph: the decode for the (fixed) shape is captured once into a hipGraph on static buffers and replayed, as the product loop treats
    the UNet body; re-captured when the shape or the decoder's workspace changes.  Eager and replayed results are bit-identical."""

    def __init__(self, taesd, on_image: Callable[[int, torch.Tensor], None], source: str = "x", rows: slice = slice(0, 1), every: int = 1,
                 use_graph: bool = True):
        if source not in ("x", "denoised"):
            raise ValueError("source must be 'x' or 'denoised'")
        if every < 1:
            raise ValueError("every must be >= 1")
        self.taesd, self.on_image, self.source, self.rows, self.every, self.use_graph = taesd, on_image, source, rows, int(every), use_graph
        self.calls = 0
        self._key = self._shape = None
        self._graph = None
        self._lat = self._f32 = self._u8 = self._host = self._event = None

    def reset(self) -> None:
        self.calls = 0

    def _buffers(self, shape) -> None:
        """Static device buffers, the pinned host image and the copy's event for a latent of `shape` = (R, 4, h, w)."""
        r, _, h, w = shape
        dev = self.taesd.device
        with torch.inference_mode(False):      # plain tensors whatever mode the first call came in (the reference samples under inference_mode)
            self._lat = torch.zeros(r, h, w, 4, dtype=torch.float32, device=dev)
            self._f32 = torch.empty(r, 8 * h, 8 * w, 3, dtype=torch.float32, device=dev)
            self._u8 = torch.empty(r, 8 * h, 8 * w, 3, dtype=torch.uint8, device=dev)
            self._host = torch.empty(r, 8 * h, 8 * w, 3, dtype=torch.uint8, pin_memory=True)
        self._event = torch.cuda.Event()
        self._graph = None

    def _body(self) -> None:
        self.taesd.decode_into(self._lat, self._f32, self._u8)

    def _capture(self) -> None:
        """pipeline.GraphedBody's capture (warm-up on a side stream, thread-local error mode); that class keys on a UNet's state."""
        dev = self.taesd.device
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            self._body()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            self._body()
        self._graph = g

    def _image_device(self, lat: torch.Tensor) -> torch.Tensor:
        """lat [R, 4, h, w] on the decoder's device -> the pinned host image [R, 8h, 8w, 3] uint8, complete on return."""
        shape = tuple(lat.shape)
        if self._lat is None or shape != self._shape:
            self._buffers(shape)
            self._shape = shape
        with torch.cuda.device(self.taesd.device):
            self._lat.copy_(lat.permute(0, 2, 3, 1))
            if self.use_graph:
                if self._graph is None or self._key != (shape, self.taesd.reserve_epoch):
                    self._capture()                                   # (its warm-up grows the workspace where the shape needs it)
                    self._key = (shape, self.taesd.reserve_epoch)
                self._graph.replay()
            else:
                self._body()
            self._host.copy_(self._u8, non_blocking=True)
            self._event.record()
            self._event.synchronize()
        return self._host

    def __call__(self, d: dict) -> None:
        self.calls += 1
        if self.calls % self.every:
            return
        lat = d.get(self.source)
        if lat is None:
            lat = d["x"]
        lat = lat[self.rows]
        if lat.is_cuda:
            image = self._image_device(lat.to(self.taesd.device, torch.float32)).clone()
        else:                                   # a decoder that lives on the host (the tests' stand-in): nothing to stage
            image = self.taesd.image(lat).to("cpu", torch.uint8)
        self.on_image(int(d["i"]), image)
