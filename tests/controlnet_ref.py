"""fp32 restatement of upstream ComfyUI's ControlNet on the blocks of oracle/sd15_ref.py (helper module of the ControlNet tests).

  hint_encoder        cldm.ControlNet.input_hint_block: eight 3x3 pad-1 convolutions, SiLU behind all but the last, stride 2 at the third, fifth, seventh
  controlnet_forward  cldm.ControlNet.forward: h = input_blocks[0](x) + hint; one zero convolution per input block, middle_block_out behind the
                      middle block -> the residuals, len(input blocks) + 1 of them
  unet_forward        oracle.sd15_ref.unet_forward with `control` where the reference calls apply_control1 (LD.py:5290, 5742, 5747) and upstream
                      adds: control["middle"] behind the middle block, control["output"].pop() to every hs.pop() — residual i joins hs[i]
  apply_model         BaseModel.apply_model around both (EPS input scaling, the timestep lookup, denoised = x - eps sigma)
The residuals passed as `control` are already scaled by the strength, as upstream's control_merge scales them.
"""
from __future__ import annotations

import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lightdiffusion_amd import weights as W      # noqa: E402
from oracle import sd15_ref as O                 # noqa: E402


def synth_state_dict(cfg: dict, seed: int = 0, hint_channels: int = 3) -> dict:
    """the synthetic ControlNet's fp32 masters (weights.synth_controlnet_tensor), bare cldm names"""
    return {k: W.synth_controlnet_tensor(k, s, seed) for k, s in W.controlnet_param_shapes(cfg, hint_channels).items()}


def hint_encoder(sd: dict, hint: torch.Tensor) -> torch.Tensor:
    """hint [hb, hint_channels, 8h, 8w] -> [hb, model_channels, h, w]"""
    h = hint
    for i, stride in enumerate(W.HINT_STRIDES):
        h = O._conv(h, sd, f"input_hint_block.{2 * i}", stride=stride)
        if i != len(W.HINT_STRIDES) - 1:
            h = F.silu(h)
    return h


def _emb(sd, cfg, t, dtype):
    return O._lin(F.silu(O._lin(O.timestep_embedding(t, cfg["model_channels"]).to(dtype), sd, "time_embed.0")), sd, "time_embed.2")


def _run(sd, cfg, layers, h, emb, ctx, out_hw=None):
    for kind, p in layers:
        if kind == "conv":
            h = O._conv(h, sd, p)
        elif kind == "res":
            h = O.resblock(h, emb, sd, p)
        elif kind == "st":
            h = O.spatial_transformer(h, ctx, sd, p, cfg["num_heads"])
        elif kind == "down":
            h = O._conv(h, sd, p, stride=2)
        elif kind == "up":
            size = out_hw if out_hw is not None else (h.shape[2] * 2, h.shape[3] * 2)
            h = O._conv(F.interpolate(h, size=size, mode="nearest"), sd, p)
    return h


def controlnet_forward(sd: dict, cfg: dict, x: torch.Tensor, hint: torch.Tensor, t: torch.Tensor, ctx: torch.Tensor) -> list:
    """cldm.ControlNet.forward: x [N,4,h,w] (already scaled), hint [1 or N, hc, 8h, 8w], t [N] timestep indices as float, ctx [N,L,D] -> the
    residuals [N, C_i, H_i, W_i]; the last one is the middle block's."""
    plan = O.unet_plan(cfg)
    emb = _emb(sd, cfg, t, x.dtype)
    guided = hint_encoder(sd, hint)
    outs, h = [], x
    for i, layers in enumerate(plan["input"]):
        h = _run(sd, cfg, layers, h, emb, ctx)
        if guided is not None:
            h = h + guided                               # (a batch-1 hint broadcasts over the batch)
            guided = None
        outs.append(O._conv(h, sd, f"zero_convs.{i}.0", padding=0))
    h = _run(sd, cfg, plan["middle"], h, emb, ctx)
    outs.append(O._conv(h, sd, "middle_block_out.0", padding=0))
    return outs


def unet_forward(sd: dict, cfg: dict, x, t, ctx, control=None) -> torch.Tensor:
    """UNetModel1.forward with upstream's apply_control: control = residuals as controlnet_forward returns them (scaled by the strength)"""
    plan = O.unet_plan(cfg)
    emb = _emb(sd, cfg, t, x.dtype)
    hs, h = [], x
    for layers in plan["input"]:
        h = _run(sd, cfg, layers, h, emb, ctx)
        hs.append(h)
    h = _run(sd, cfg, plan["middle"], h, emb, ctx)
    output = None
    if control is not None:
        h = h + control[-1]
        output = list(control[:-1])
    for layers in plan["output"]:
        hsp = hs.pop()
        if output is not None:
            hsp = hsp + output.pop()
        h = torch.cat([h, hsp], dim=1)
        h = _run(sd, cfg, layers, h, emb, ctx, tuple(hs[-1].shape[2:]) if hs else None)
    return O._conv(F.silu(O._gn(h, sd, "out.0", 1e-5)), sd, "out.2")


def control_residuals(cn_sd, cfg, ms, x, sigma, ctx, hint) -> list:
    """the control branch as the sampler calls it: on the UNet's scaled input and timestep"""
    s = sigma.view(-1, 1, 1, 1)
    xc = x / (s ** 2 + ms.sigma_data ** 2) ** 0.5
    return controlnet_forward(cn_sd, cfg, xc, hint, ms.timestep(sigma).float(), ctx)


def apply_model(sd, cfg, ms, x, sigma, ctx, cn_sd=None, hint=None, strength: float = 1.0, eps_only: bool = False) -> torch.Tensor:
    """BaseModel.apply_model (LD.py:5828-5860) with a ControlNet (cn_sd, hint): denoised x0 (or the raw eps)"""
    s = sigma.view(-1, 1, 1, 1)
    xc = x / (s ** 2 + ms.sigma_data ** 2) ** 0.5
    t = ms.timestep(sigma).float()
    control = None
    if cn_sd is not None:
        control = [r * strength for r in controlnet_forward(cn_sd, cfg, xc, hint, t, ctx)]
    eps = unet_forward(sd, cfg, xc, t, ctx, control)
    return eps if eps_only else x - eps * s
