"""ControlNet's control branch as a chain of operator calls (helper module of tests/test_controlnet_chain_gpu.py).

A plain restatement of upstream ComfyUI's cldm.ControlNet.forward (tests/controlnet_ref.py states it in fp32): the hint encoder
(input_hint_block: eight 3x3 convolutions, SiLU behind all but the last, stride 2 at the third, fifth and seventh), then the UNet's time
embedding, input blocks and middle block with h = conv_in(x) + hint, one 1x1 zero convolution per input block and middle_block_out behind the
middle block — every step ONE call of the operator seam on the synthetic ControlNet's weights.  The ResBlock, the transformer, the context,
the time embedding, conv_in and the downsampling are tests/unet_chain.py's UNetChain, unchanged; what is added here is the hint, the add and
the zero convolutions.  The controlled UNet is UNetChain.forward(..., control=(residuals, r_n, strength)).  Nothing here reads the executor.

A CFG pair shares no prefix in the control branch: conv_in runs once per latent and stores both halves (dup_off), everything behind it runs
on all 2B samples.
"""
from __future__ import annotations

import torch

from chain_harness import Feat
from lightdiffusion_amd import weights as W
from unet_chain import UNetChain, modules


class ControlChain(UNetChain):
    shares_prefix = False

    def __init__(self, cfg: dict, device="cuda:0", seed: int = 0, hint_channels: int = 3):
        self.read = set()          # every parameter name a call asked for (the completeness test's)
        super().__init__(cfg, device, seed, shapes=W.controlnet_param_shapes(cfg, hint_channels), prefix=W.CONTROL_NAME_PREFIX)
        self.hint = None
        self.residuals = []

    def block_list(self, cfg):
        return [b for b in modules(cfg) if b[0][0] != "output"]

    def master(self, name):
        self.read.add(name)
        return super().master(name)

    # -- cldm.ControlNet.input_hint_block
    def set_hint(self, image: torch.Tensor) -> torch.Tensor:
        """image fp32 NCHW [hb][hint_channels][8 h][8 w] -> the encoded hint fp16 [hb][h][w][model_channels]; its taps replace the chain's."""
        ops = self.ops
        self.taps = []
        a = image.to(self.dev, torch.float32).contiguous()
        for i, stride in enumerate(W.HINT_STRIDES):
            name = f"input_hint_block.{2 * i}"
            silu = i != len(W.HINT_STRIDES) - 1
            wt, b = self.conv3(name + ".weight"), self.vec(name + ".bias")
            y = ops.hint_conv(a, wt, b, stride=stride, silu=silu)
            self.tap("hint_conv", name, dict(x=a), dict(w=self.oihw(name + ".weight"), b=b, stride=stride, silu=silu), y)
            a = y
        self.hint = a
        self.hint_taps = self.taps
        return a

    # -- behind input block 0: h = conv_in(x) + hint; behind every input block: its zero convolution; behind the middle block: middle_block_out
    def block_done(self, where, bi, f: Feat) -> Feat:
        ops = self.ops
        if where == "input" and bi == 0:
            assert self.hint is not None and self.hint.shape[1:3] == f.t.shape[1:3], "set_hint for this latent size first"
            h = f.t.clone()                            # (the sum goes into a copy: conv_in's tap keeps the tensor it wrote)
            ops.control_add_([h], [self.hint], 1.0, r_n=self.hint.shape[0])
            self.tap("control_add", "input_blocks.0.0+hint", dict(t=[f.t], r=[self.hint]), dict(strength=1.0, r_n=self.hint.shape[0]), (h,))
            f = Feat(h)
        name = f"zero_convs.{bi}.0" if where == "input" else "middle_block_out.0"
        wz, bz = self.mat(name + ".weight"), self.vec(name + ".bias")
        r = ops.conv2d(f.t, wz, bz, ksize=1)
        self.tap("conv", name, dict(x=f.t), dict(w=self.oihw(name + ".weight"), b=bz), r, n=f.t.shape[0])
        self.residuals.append(r)
        return f

    def forward(self, x: torch.Tensor, sigma: torch.Tensor, pair: bool = False):
        """-> the 13 residuals, fp16 [n or 2 (n / 2)][H][W][C]; the last one is the middle block's."""
        self.residuals = []
        return super().forward(x, sigma, pair=pair)

    def finish(self, f, x, sigma, eps_only, in_mod):
        return list(self.residuals)
