"""ESRGAN upscaler on one MI355X: the object `UpscaleModelLoader` returns and `ImageUpscaleWithModel` applies tile by tile
(LD.py:7240-7272, 7356-7395).  `MI355XUpscaler` owns an `ld_esrgan` handle (RRDBNet on the dense-block HIP kernel); `tiled_upscale` is
`tiled_scale` (LD.py:7282-7353) with the feather blend on the device: only the two 1-D ramps of a tile are built on the host.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Tuple

import torch

from . import weights as W
from ._lib import ESRGANConfig, check, lib
from ._model import ResidentModel, WeightSource, _stream


def tile_plan(height: int, width: int, tile: int, overlap: int) -> List[Tuple[int, int, int, int]]:
    """(y, x, h, w) of every tile tiled_scale visits (LD.py:7321-7323): starts at range(0, size, tile - overlap), clipped at the edge."""
    step = tile - overlap
    if step <= 0:
        raise ValueError("tile must be larger than overlap")
    return [(y, x, min(tile, height - y), min(tile, width - x)) for y in range(0, height, step) for x in range(0, width, step)]


def feather_ramp(n: int, feather: int) -> torch.Tensor:
    """One axis of tiled_scale's mask for an upscaled tile of n pixels (LD.py:7327-7336): (t + 1) / feather for t < feather from BOTH
    ends, multiplied where the two ramps overlap (n < 2 feather).  fp32, in the reference's order of operations."""
    m = torch.ones(n, dtype=torch.float32)
    for t in range(feather):
        f = (1.0 / feather) * (t + 1)
        m[t:1 + t] *= f
        m[n - 1 - t:n - t] *= f
    return m


class MI355XUpscaler(ResidentModel):
    """RRDBNet resident on one MI355X.  `cfg`: in_nc, out_nc, nf, gc, nb, scale (checkpoint.detect_esrgan_config); `weights`: a state
    dict with old-arch keys (checkpoint.normalize_esrgan_keys) or a callable (name, shape) -> tensor."""

    family = "esrgan"

    def __init__(self, cfg: dict, weights: WeightSource, device="cuda:0", max_batch: int = 1, max_hw=(64, 64)):
        self.cfg = dict(cfg)
        self.device = torch.device(device)
        c = ESRGANConfig()
        c.in_nc, c.out_nc, c.nf, c.gc, c.nb, c.scale = (int(cfg[k]) for k in ("in_nc", "out_nc", "nf", "gc", "nb", "scale"))
        self.scale = int(cfg["scale"])
        self._create(weights, C.byref(c))
        self._ensure(max_batch, max_hw[0], max_hw[1])

    def _io(self, image: torch.Tensor):
        x = image.to(self.device, torch.float32).contiguous()
        if x.dim() != 4 or x.shape[-1] != 3:
            raise ValueError(f"expected an image batch [B, H, W, 3], got {tuple(image.shape)}")
        b, h, w, _ = x.shape
        self._ensure(b, h, w)
        return x, torch.empty(b, h * self.scale, w * self.scale, 3, dtype=torch.float32, device=self.device), b, h, w

    def forward_device(self, image: torch.Tensor) -> torch.Tensor:
        """[B, H, W, 3] fp32 -> the model's raw (unclamped) output [B, H s, W s, 3] fp32 on the device."""
        x, out, b, h, w = self._io(image)
        with torch.cuda.device(self.device):
            check(lib().ld_esrgan_forward(self._h, x.data_ptr(), out.data_ptr(), b, h, w, _stream()), "ld_esrgan_forward")
        return out

    def profile(self, image: torch.Tensor) -> list:
        """One forward with HIP events around every launch -> [(what, dims, flops, microseconds, kernel)] in launch order."""
        x, out, b, h, w = self._io(image)
        with torch.cuda.device(self.device):
            check(lib().ld_esrgan_profile(self._h, x.data_ptr(), out.data_ptr(), b, h, w, _stream()), "ld_esrgan_profile")
        return self.profile_launches()

    def to(self, device):
        """The reference moves the model to the device before and to the CPU after an upscale (LD.py:7365, 7393); the weights here stay
        resident in the C handle."""
        return self


def blend_tile(ps: Optional[torch.Tensor], my: Optional[torch.Tensor], mx: Optional[torch.Tensor], out: torch.Tensor, div: torch.Tensor,
               y0: int = 0, x0: int = 0) -> None:
    """out[y0:, x0:] += ps * my x mx, div[y0:, x0:] += my x mx on the device (`ld_op_tile_blend`); ps None: the final out /= div.
    ps [th, tw, c], out [OH, OW, c], div [OH, OW], all fp32 and contiguous on one device."""
    oh, ow, c = out.shape
    with torch.cuda.device(out.device):
        if ps is None:
            check(lib().ld_op_tile_blend(None, None, None, 0, 0, out.data_ptr(), div.data_ptr(), oh, ow, 0, 0, c, _stream()), "ld_op_tile_blend")
        else:
            th, tw, _ = ps.shape
            check(lib().ld_op_tile_blend(ps.data_ptr(), my.data_ptr(), mx.data_ptr(), th, tw, out.data_ptr(), div.data_ptr(), oh, ow, y0, x0, c,
                                         _stream()), "ld_op_tile_blend")


def tiled_upscale(model: MI355XUpscaler, image: torch.Tensor, tile: int = 512, overlap: int = 32) -> torch.Tensor:
    """tiled_scale (LD.py:7282-7353) of an image batch [B, H, W, 3] on the device: the unclamped blend [B, H s, W s, 3] fp32."""
    s = model.scale
    img = image.to(model.device, torch.float32)
    B, H, Wd, _ = img.shape
    feather = round(overlap * s)
    out = torch.zeros(B, H * s, Wd * s, 3, dtype=torch.float32, device=model.device)
    div = torch.zeros(B, H * s, Wd * s, dtype=torch.float32, device=model.device)
    ramps = {}
    for b in range(B):
        for (y, x, h, w) in tile_plan(H, Wd, tile, overlap):
            ps = model.forward_device(img[b:b + 1, y:y + h, x:x + w])[0]
            for n in (h * s, w * s):
                if n not in ramps:
                    ramps[n] = feather_ramp(n, feather).to(model.device)
            blend_tile(ps, ramps[h * s], ramps[w * s], out[b], div[b], y * s, x * s)
        blend_tile(None, None, None, out[b], div[b])
    return out
