"""RRDBNet's forward as a chain of operator calls (helper module of tests/test_esrgan_chain_gpu.py).

A plain restatement of RRDBNet.forward (LD.py:7141-7149) over the modules its constructor builds (LD.py:7092-7139): conv_first, the
ShortcutBlock around nb RRDBs and the trunk convolution (LD.py:6787-6789), each RRDB three ResidualDenseBlock_5C with `out * 0.2 + x`
(LD.py:6902), each block five conv_blocks with `x5 * 0.2 + x` (LD.py:6905-6992), log2(scale) upconv_blocks (LD.py:6995-7022), the HR
convolution and conv_last — the LD.py lines tests/esrgan_ref.py restates — with ONE call of the operator seam (lightdiffusion_amd/ops.py)
per launch of the executor (csrc/esrgan.hip esrgan_run), on weights taken from the synthetic checkpoint and brought into the resident
layout by the seam's own repack operator.  Nothing here reads the executor: the chain is what tests/test_esrgan_chain_gpu.py diffs it
against, launch by launch and bit by bit, and every call leaves a tap from which the test recomputes that one stage in fp64.

The chain keeps the executor's buffer semantics in torch tensors of its own: two dense buffers of pitch nf + 4 gc = 192 that alternate
(convolutions 1-4 of a block append their 32 channels IN PLACE behind the channels they read, into a buffer that still holds the block
before last's x1 .. x4; convolution 5 reads R1 from channels 0 .. 63 of its own input buffer and writes the other buffer), the RRDB input
as R2 of every third block, which the same call overwrites through the second store (y2 == r2), the trunk input, and a clone where the
executor copies.  All of them start as NaN: a channel read before the network wrote it cannot pass.

A tap: kind (first, dense, conv5, trunk, up, hr, last), name (the checkpoint's prefix), inp (every operand CLONED before the call: the
calls are in place), par (weights as the checkpoint lays them out, bias, slope, scales, c_off, cout), out (the channels written, cloned),
before / after (the whole output buffer around the call), y2 (the second store's buffer after the call), launches.

`modules(cfg)` is the host-only walk of the constructor: [(kind, name, cin, cout)] in launch order.
"""
from __future__ import annotations

import torch

from chain_harness import ChainBase
from lightdiffusion_amd import weights as W

SLOPE = 0.2           # act("leakyrelu"): nn.LeakyReLU(0.2) (LD.py:6700-6716)


def n_upconvs(scale: int) -> int:
    return int(scale).bit_length() - 1


# ------------------------------------------------------------------ the module list (host only)

def modules(cfg: dict):
    """[(kind, name, cin, cout)] in forward order: one entry per convolution = per launch, 15 nb + 4 + log2(scale) of them (15 nb + 6 at x4)."""
    nf, gc, nb = cfg["nf"], cfg["gc"], cfg["nb"]
    mods = [("first", "model.0", cfg["in_nc"], nf)]
    for b in range(nb):
        for r in (1, 2, 3):
            for k in range(5):
                mods.append(("dense" if k < 4 else "conv5", f"model.1.sub.{b}.RDB{r}.conv{k + 1}.0", nf + k * gc, gc if k < 4 else nf))
    mods.append(("trunk", f"model.1.sub.{nb}", nf, nf))
    n_up = n_upconvs(cfg["scale"])
    mods += [("up", f"model.{3 * (u + 1)}", nf, nf) for u in range(n_up)]
    mods += [("hr", f"model.{3 * n_up + 2}", nf, nf), ("last", f"model.{3 * n_up + 4}", nf, cfg["out_nc"])]
    return mods


# ------------------------------------------------------------------ the chain

class ESRGANChain(ChainBase):
    def __init__(self, cfg: dict, device="cuda:0", seed: int = 0):
        super().__init__(W.esrgan_param_shapes(cfg), device, seed)
        self.cfg = dict(cfg)

    def _buf(self, n, h, w, c):
        return torch.full((n, h, w, c), float("nan"), dtype=torch.float16, device=self.dev)

    def _conv(self, kind, name, x, cin, y, c_off, cout, slope=0.0, r1=None, s1=1.0, r2=None, s2=1.0, y2=None, up=False):
        """One conv_block: one call of ops.esrgan_conv and its tap."""
        inp = dict(x=x[..., :cin].clone(), r1=None if r1 is None else r1[..., :cout].clone(), r2=None if r2 is None else r2[..., :cout].clone())
        before = y.clone()
        self.ops.esrgan_conv(x, cin, self.conv3(name + ".weight"), self.vec(name + ".bias"), y, c_off, cout, slope=slope, r1=r1, s1=s1, r2=r2, s2=s2,
                             y2=y2, up=up)
        par = dict(w=self.oihw(name + ".weight"), b=self.vec(name + ".bias"), slope=slope, s1=s1, s2=s2, c_off=c_off, cout=cout, up=up)
        self.taps.append(dict(kind=kind, name=name, inp=inp, par=par, out=y[..., c_off:c_off + cout].clone(), before=before, after=y.clone(),
                              y2=None if y2 is None else y2.clone(), launches=self.ops.last_launches()))

    def forward(self, image: torch.Tensor) -> torch.Tensor:
        """image [n][h][w][3] fp32 -> the model's raw output [n][h s][w s][3] fp32 on the device."""
        ops, cfg = self.ops, self.cfg
        self.taps = []
        x = image.to(self.dev, torch.float32).contiguous()
        n, h, w, _ = x.shape
        nf, gc, nb = cfg["nf"], cfg["gc"], cfg["nb"]
        ldd = nf + 4 * gc
        dense = [self._buf(n, h, w, ldd), self._buf(n, h, w, ldd)]
        trunk_in = self._buf(n, h, w, nf)

        # conv_first: the trunk's input, and the first RRDB's (dense buffer 0 and the ShortcutBlock's residual)
        before = dense[0].clone()
        ops.esrgan_first(x, self.conv3("model.0.weight"), self.vec("model.0.bias"), dense[0], trunk_in)
        self.taps.append(dict(kind="first", name="model.0", inp=dict(x=x), par=dict(w=self.conv3("model.0.weight"), b=self.vec("model.0.bias"), c_off=0, cout=nf),
                              out=dense[0][..., :nf].clone(), before=before, after=dense[0].clone(), y2=trunk_in.clone(), launches=ops.last_launches()))
        rrdb_in = trunk_in.clone()                      # (the executor's device-to-device copy)
        cur = 0
        for b in range(nb):
            for r in (1, 2, 3):
                d = dense[cur]
                base = f"model.1.sub.{b}.RDB{r}.conv"
                for k in range(4):                      # x_k = lrelu(conv_k(cat(x, x_1 .. x_{k-1}))), appended in place
                    cin = nf + k * gc
                    self._conv("dense", f"{base}{k + 1}.0", d, cin, d, cin, gc, slope=SLOPE)
                # x5 * 0.2 + x; the RRDB's third block also carries out * 0.2 + x and leaves the sum as the next RRDB's input
                last = r == 3
                self._conv("conv5", f"{base}5.0", d, ldd, dense[cur ^ 1], 0, nf, r1=d, s1=0.2, r2=rrdb_in if last else None, s2=0.2,
                           y2=rrdb_in if last else None)
                cur ^= 1
        f = dense[cur ^ 1]
        self._conv("trunk", f"model.1.sub.{nb}", dense[cur], nf, f, 0, nf, r1=trunk_in, s1=1.0)      # trunk convolution + the ShortcutBlock's add
        H, Wd = h, w
        n_up = n_upconvs(cfg["scale"])
        for u in range(n_up):                           # nearest 2x + convolution + LeakyReLU
            H, Wd = 2 * H, 2 * Wd
            g = self._buf(n, H, Wd, nf)
            self._conv("up", f"model.{3 * (u + 1)}", f, nf, g, 0, nf, slope=SLOPE, up=True)
            f = g
        hr = self._buf(n, H, Wd, nf)
        self._conv("hr", f"model.{3 * n_up + 2}", f, nf, hr, 0, nf, slope=SLOPE)
        name = f"model.{3 * n_up + 4}"
        out = ops.esrgan_last(hr, self.conv3(name + ".weight"), self.vec(name + ".bias"))
        self.taps.append(dict(kind="last", name=name, inp=dict(x=hr.clone()), par=dict(w=self.conv3(name + ".weight"), b=self.vec(name + ".bias")), out=out,
                              before=None, after=None, y2=None, launches=ops.last_launches()))
        return out
