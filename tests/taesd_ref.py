"""Own-words torch restatement of TAESD's decoder from Decoder2's state dict (the keys of taesd_decoder.safetensors), functional conv2d.
Helper module of the preview tests and of tools/preview_time.py; tests/test_preview_cpu.py pins it against the reference's goldens.

    t = relu(conv(3 tanh(x / 3); 1))
    three stages s = 0, 1, 2:  Block 3 + 5s, Block 4 + 5s, Block 5 + 5s, nearest 2x, conv(.; 7 + 5s) without bias
    Block 18, conv(.; 19);  decode = (. - 0.5) * 2
    Block i (t) = relu(conv(relu(conv(relu(conv(t; i.conv.0)); i.conv.2)); i.conv.4) + t)
every convolution 3x3, pad 1.  The preview image of a decode d is uint8(clip(255 ((d + 1) * 0.5), 0, 255)), fp32 in that order, truncated.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F


def decode(sd, latent: torch.Tensor, dtype=torch.float32, channels_last: bool = False) -> torch.Tensor:
    """sd: Decoder2's keys; latent [B, 4, h, w] -> TAESD.decode as NHWC [B, 8h, 8w, 3] in `dtype` on the latent's device."""
    dev = latent.device
    sd = {k: v.to(dev, dtype) for k, v in sd.items()}
    if channels_last:
        sd = {k: (v.contiguous(memory_format=torch.channels_last) if v.dim() == 4 else v) for k, v in sd.items()}
    x = latent.to(dtype)
    x = x.contiguous(memory_format=torch.channels_last) if channels_last else x.contiguous()
    conv = lambda t, p: F.conv2d(t, sd[p + ".weight"], sd.get(p + ".bias"), padding=1)

    def block(t, i):
        u = F.relu(conv(t, f"{i}.conv.0"))
        u = F.relu(conv(u, f"{i}.conv.2"))
        return F.relu(conv(u, f"{i}.conv.4") + t)

    t = F.relu(conv(torch.tanh(x / 3) * 3, "1"))
    for s in range(3):
        for j in range(3):
            t = block(t, 3 + 5 * s + j)
        t = conv(F.interpolate(t, scale_factor=2, mode="nearest"), str(7 + 5 * s))
    t = conv(block(t, 18), "19")
    return ((t - 0.5) * 2).permute(0, 2, 3, 1).contiguous()


def to_image(d: torch.Tensor) -> torch.Tensor:
    """A decode -> the preview image, uint8, same shape: fp32 (d + 1) * 0.5, times 255, clipped, truncated."""
    return (255.0 * ((d.float() + 1.0) * 0.5)).clamp(0.0, 255.0).to(torch.uint8)
