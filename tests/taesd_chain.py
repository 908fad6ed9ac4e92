"""TAESD's decoder as a chain of operator calls (helper module of tests/test_taesd_chain_gpu.py).

A plain restatement of Decoder2 / TAESD.decode (LD.py:688-754: Clamp, the first convolution + ReLU, three stages of three Blocks, an
nn.Upsample and a bias-free convolution, one more Block, the last convolution, and decode's (. - 0.5) * 2) — the LD.py lines
tests/taesd_ref.py restates — with ONE call of the operator seam (lightdiffusion_amd/ops.py) per launch of the executor (csrc/taesd.hip
taesd_run), on weights taken from the synthetic checkpoint and brought into the resident layout by the seam's own repack operator.  Nothing
here reads the executor: the chain is what tests/test_taesd_chain_gpu.py diffs it against, launch by launch and bit by bit, and every call
leaves a tap from which the test recomputes that one stage in fp64.

The chain keeps the executor's buffer semantics in torch tensors of its own: three flat buffers of the OUTPUT resolution (64 h w pixels of
64 channels) that rotate and are viewed at 1/8, 1/4, 1/2 and full resolution; a Block reads x = buf[cur], writes t1 = buf[cur + 1],
t2 = buf[cur + 2], and its third convolution reads t2, adds x and writes over t1; an upsampling convolution reads buf[cur] at the old size
and writes buf[cur + 1] at the new one.  All three start as NaN: an element read before the network wrote it cannot pass.

A tap: kind (first, conv, up, last), name (the state dict's prefix), inp (every operand CLONED before the call), par (weights as the
checkpoint lays them out, bias or None, relu), out (cloned), image (the last convolution's uint8 output), launches.

`modules()` is the host-only walk of Decoder2's Sequential: [(kind, name, cin, cout)] in launch order, 35 entries.
"""
from __future__ import annotations

import torch

from chain_harness import ChainBase
from lightdiffusion_amd import weights as W

PREFIX = "taesd_decoder."       # nodes.load_synthetic_taesd seeds the synthetic tensors under the whole module's key


def modules():
    """[(kind, name, cin, cout)] in forward order, one entry per convolution = per launch."""
    mods = [("first", "1", 4, 64)]
    block = lambda i: [("conv", f"{i}.conv.{k}", 64, 64) for k in (0, 2, 4)]
    for s in range(3):
        for j in range(3):
            mods += block(3 + 5 * s + j)
        mods.append(("up", str(7 + 5 * s), 64, 64))
    mods += block(18)
    mods.append(("last", "19", 64, 3))
    return mods


class TAESDChain(ChainBase):
    def __init__(self, device="cuda:0", seed: int = 0):
        super().__init__(W.taesd_decoder_param_shapes(), device, seed, prefix=PREFIX)

    def decode(self, latent: torch.Tensor):
        """latent [n][4][h][w] -> (TAESD.decode as NHWC [n][8h][8w][3] fp32, the preview image uint8 of the same shape) on the device."""
        ops = self.ops
        self.taps = []
        x = latent.to(self.dev, torch.float32).permute(0, 2, 3, 1).contiguous()
        n, h, w, _ = x.shape
        flat = [torch.full((n * 64 * h * w * 64,), float("nan"), dtype=torch.float16, device=self.dev) for _ in range(3)]
        H, Wd, cur = h, w, 0
        view = lambda i, hh, ww: flat[i % 3][:n * hh * ww * 64].view(n, hh, ww, 64)

        def conv(kind, name, src, dst, residual=None, relu=False, up=False, bias=True):
            inp = dict(x=src.clone(), residual=None if residual is None else residual.clone())
            b = self.vec(name + ".bias") if bias else None
            ops.taesd_conv(src, self.conv3(name + ".weight"), b, dst, residual=residual, relu=relu, up=up)
            self.taps.append(dict(kind=kind, name=name, inp=inp, par=dict(w=self.oihw(name + ".weight"), b=b, relu=relu, up=up), out=dst.clone(),
                                  launches=ops.last_launches()))

        def block(i):                                   # relu(conv(relu(conv(relu(conv(x))))) + x)
            nonlocal cur
            xb, t1, t2 = view(cur, H, Wd), view(cur + 1, H, Wd), view(cur + 2, H, Wd)
            conv("conv", f"{i}.conv.0", xb, t1, relu=True)
            conv("conv", f"{i}.conv.2", t1, t2, relu=True)
            conv("conv", f"{i}.conv.4", t2, t1, residual=xb, relu=True)
            cur = (cur + 1) % 3

        y0 = view(0, h, w)
        ops.taesd_first(x, self.conv3("1.weight"), self.vec("1.bias"), y0)
        self.taps.append(dict(kind="first", name="1", inp=dict(x=x), par=dict(w=self.conv3("1.weight"), b=self.vec("1.bias")), out=y0.clone(),
                              launches=ops.last_launches()))
        for s in range(3):
            for j in range(3):
                block(3 + 5 * s + j)
            src = view(cur, H, Wd)
            H, Wd = 2 * H, 2 * Wd                        # nn.Upsample(scale_factor=2) + the bias-free convolution
            conv("up", str(7 + 5 * s), src, view(cur + 1, H, Wd), up=True, bias=False)
            cur = (cur + 1) % 3
        block(18)
        last = view(cur, H, Wd)
        out, img = ops.taesd_last(last, self.conv3("19.weight"), self.vec("19.bias"), image=True)
        self.taps.append(dict(kind="last", name="19", inp=dict(x=last.clone()), par=dict(w=self.conv3("19.weight"), b=self.vec("19.bias")), out=out, image=img,
                              launches=ops.last_launches()))
        return out, img
