"""Own-words torch restatement of RRDBNet (ESRGAN) from an old-arch state dict, NHWC in and out, functional conv2d.  Helper module of the
upscaler tests and of tools/upscale_time.py; tests/test_upscale_cpu.py pins it against the reference's goldens.

    fea   = conv(x; model.0)
    trunk = RRDB_0 .. RRDB_{nb-1}(fea), then conv(.; model.1.sub.nb);            out = fea + trunk
    RRDB(x)  = RDB3(RDB2(RDB1(x))) * 0.2 + x
    RDB(x)   : x_k = lrelu(conv_k(cat(x, x_1 .. x_{k-1})), 0.2) for k = 1 .. 4;  x_5 = conv_5(cat(x, x_1 .. x_4));  x_5 * 0.2 + x
    log2(scale) times: nearest 2x, conv (model.3, model.6, ..), lrelu 0.2;  then lrelu(conv(HR), 0.2), conv(last)
"""
from __future__ import annotations

import torch
import torch.nn.functional as F


def n_upconvs(scale: int) -> int:
    return int(scale).bit_length() - 1


def _same(t: torch.Tensor) -> torch.Tensor:
    return t


def half_round(t: torch.Tensor) -> torch.Tensor:
    return t.half().to(t.dtype)


def dense_block(sd, prefix: str, x: torch.Tensor, rnd=_same) -> torch.Tensor:
    feats = [x]
    for k in range(1, 6):
        y = rnd(F.conv2d(torch.cat(feats, 1), sd[f"{prefix}.conv{k}.0.weight"], sd[f"{prefix}.conv{k}.0.bias"], padding=1))
        if k < 5:
            feats.append(rnd(F.leaky_relu(y, 0.2)))
    return y * 0.2 + x


def rrdbnet(sd, x_nhwc: torch.Tensor, nb: int, scale: int, dtype=torch.float32, channels_last: bool = False, emulate_fp16: bool = False) -> torch.Tensor:
    """sd: old-arch keys; x_nhwc [B, H, W, 3] -> [B, H s, W s, 3] (unclamped) in `dtype` on x's device.
    emulate_fp16: the emulation the fixtures' `emul_rel_l2` was measured with (tools/make_upscale_golden.py): weights, the input and every
    Conv2d / LeakyReLU output rounded to fp16 — where the device path rounds — and everything else in `dtype`."""
    dev = x_nhwc.device
    rnd = half_round if emulate_fp16 else _same
    sd = {k: rnd(v.to(dev, dtype)) for k, v in sd.items()}
    x_nhwc = rnd(x_nhwc.to(dtype))
    if channels_last:
        sd = {k: (v.contiguous(memory_format=torch.channels_last) if v.dim() == 4 else v) for k, v in sd.items()}
    x = x_nhwc.to(dtype).permute(0, 3, 1, 2)
    x = x.contiguous(memory_format=torch.channels_last) if channels_last else x.contiguous()
    conv = lambda t, p: rnd(F.conv2d(t, sd[p + ".weight"], sd[p + ".bias"], padding=1))
    lrelu = lambda t: rnd(F.leaky_relu(t, 0.2))
    fea = conv(x, "model.0")
    t = fea
    for b in range(nb):
        r = t
        for j in (1, 2, 3):
            r = dense_block(sd, f"model.1.sub.{b}.RDB{j}", r, rnd)
        t = r * 0.2 + t
    t = fea + conv(t, f"model.1.sub.{nb}")
    n_up = n_upconvs(scale)
    for u in range(n_up):
        t = lrelu(conv(F.interpolate(t, scale_factor=2, mode="nearest"), f"model.{3 * (u + 1)}"))
    t = lrelu(conv(t, f"model.{3 * n_up + 2}"))
    return conv(t, f"model.{3 * n_up + 4}").permute(0, 2, 3, 1).contiguous()


def respell(sd_old, style: str, nb: int, scale: int):
    """Old-arch keys -> 'old' (as is), 'trunk' (conv_first / RRDB_trunk / trunk_conv / upconvN / HRconv) or 'body' (body / conv_body /
    conv_upN / conv_hr): the three spellings RRDBNet checkpoints come in."""
    if style == "old":
        return dict(sd_old)
    t = style == "trunk"
    n_up = n_upconvs(scale)
    out = {}
    for k, v in sd_old.items():
        p = k.split(".")
        kind = p[-1]
        if p[1] == "0":
            out[f"conv_first.{kind}"] = v
        elif p[1] == "1" and len(p) == 5:
            out[f"{'trunk_conv' if t else 'conv_body'}.{kind}"] = v
        elif p[1] == "1":
            out[f"RRDB_trunk.{p[3]}.RDB{p[4][3:]}.{p[5]}.{kind}" if t else f"body.{p[3]}.rdb{p[4][3:]}.{p[5]}.{kind}"] = v
        else:
            n = int(p[1])
            if n == 3 * n_up + 2:
                out[f"{'HRconv' if t else 'conv_hr'}.{kind}"] = v
            elif n == 3 * n_up + 4:
                out[f"conv_last.{kind}"] = v
            else:
                out[f"{'upconv' if t else 'conv_up'}{n // 3}.{kind}"] = v
    return out
