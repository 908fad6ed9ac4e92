"""The KL-VAE's decode and encode as chains of operator calls (helper module of tests/test_vae_chain_gpu.py).

A plain restatement of post_quant_conv + Decoder.forward (LD.py:3470-3473, 3857-3882) + VAE.decode's clamp and NHWC output (LD.py:6357-6381),
and of Encoder.forward (LD.py:3731-3758) + quant_conv (LD.py:3468), over the module lists Decoder.__init__ / Encoder.__init__ build, with
ResnetBlock.forward (LD.py:3560-3576), AttnBlock.forward (LD.py:3630-3642), Upsample (LD.py:3498-3511) and Downsample (LD.py:3514-3528) —
every step ONE call of the operator seam (lightdiffusion_amd/ops.py), on weights taken from the synthetic checkpoint and brought into the
resident layouts by the seam's own repack operators.  Nothing here reads the executor (csrc/vae.hip): the chain is what
tests/test_vae_chain_gpu.py diffs it against, launch by launch and bit by bit, and every call leaves a tap (stage kind, layer name, inputs,
parameters, output, kernel, launches, producer partials) from which the test recomputes that one stage in fp64.

The GroupNorm statistics travel as the executor's do: an activation is a (tensor, partials) pair (`Feat`), a producer's partials exist only
where its launch reported chunks > 0 (the halo tile's epilogue; ops.FORM_VAE), and they reach the NEXT GroupNorm of that tensor only — the
ResnetBlock's norm1 / norm2 and norm_out.  AttnBlock's norm runs its own statistics pass whatever its input carries, as vae.hip does.

`modules(cfg, encoder)` is the host-only walk of the constructor: the list of (kind, name, cin, cout) the forward runs over.
"""
from __future__ import annotations

import math

import torch

from chain_harness import ChainBase, Feat
from lightdiffusion_amd import weights as W

EPS = 1e-6            # Normalize(): GroupNorm(32, eps=1e-6) (LD.py:3931-3939)


# ------------------------------------------------------------------ the module list (host only)

def modules(cfg: dict, encoder: bool = False):
    """[(kind, name, cin, cout)] in forward order, kind in conv_in, res, attn, up, down, norm_out, conv_out, quant: the walk of
    Decoder.__init__ (LD.py:3761-3855; post_quant_conv rides on conv_in) or of Encoder.__init__ (LD.py:3649-3729; quant_conv last)."""
    ch, cm, nrb, z = cfg["ch"], cfg["ch_mult"], cfg["num_res_blocks"], cfg["z_channels"]
    mods = []
    if not encoder:
        bi = ch * cm[-1]
        mods.append(("conv_in", "decoder.conv_in", z, bi))
        mods += [("res", "decoder.mid.block_1", bi, bi), ("attn", "decoder.mid.attn_1", bi, bi), ("res", "decoder.mid.block_2", bi, bi)]
        for lvl in reversed(range(len(cm))):
            bo = ch * cm[lvl]
            for b in range(nrb + 1):
                mods.append(("res", f"decoder.up.{lvl}.block.{b}", bi, bo))
                bi = bo
            if lvl != 0:
                mods.append(("up", f"decoder.up.{lvl}.upsample.conv", bi, bi))
        mods += [("norm_out", "decoder.norm_out", bi, bi), ("conv_out", "decoder.conv_out", bi, cfg["out_ch"])]
        return mods
    bi = ch
    mods.append(("conv_in", "encoder.conv_in", cfg["out_ch"], ch))
    for lvl in range(len(cm)):
        bo = ch * cm[lvl]
        for b in range(nrb):
            mods.append(("res", f"encoder.down.{lvl}.block.{b}", bi, bo))
            bi = bo
        if lvl != len(cm) - 1:
            mods.append(("down", f"encoder.down.{lvl}.downsample.conv", bi, bi))
    mods += [("res", "encoder.mid.block_1", bi, bi), ("attn", "encoder.mid.attn_1", bi, bi), ("res", "encoder.mid.block_2", bi, bi)]
    mods += [("norm_out", "encoder.norm_out", bi, bi), ("conv_out", "encoder.conv_out", bi, 2 * z), ("quant", "quant_conv", 2 * z, 2 * z)]
    return mods


# ------------------------------------------------------------------ the chain

class VAEChain(ChainBase):
    def __init__(self, cfg: dict, device="cuda:0", with_encoder: bool = False, seed: int = 0, source=None):
        shapes = dict(W.vae_decoder_param_shapes(cfg))
        if with_encoder:
            shapes.update(W.vae_encoder_param_shapes(cfg))
        super().__init__(shapes, device, seed, source)
        self.cfg, self.with_encoder = dict(cfg), with_encoder

    # -- ResnetBlock.forward (LD.py:3560-3576): norm1 + swish + conv1, [nin_shortcut], norm2 + swish + conv2 + the shortcut
    def resblock(self, name, f: Feat) -> Feat:
        ops = self.ops
        x = f.t
        g1, b1 = self.vec(name + ".norm1.weight"), self.vec(name + ".norm1.bias")
        g2, b2 = self.vec(name + ".norm2.weight"), self.vec(name + ".norm2.bias")
        w1, c1b = self.conv3(name + ".conv1.weight"), self.vec(name + ".conv1.bias")
        w2, c2b = self.conv3(name + ".conv2.weight"), self.vec(name + ".conv2.bias")
        h1, p1 = ops.group_norm_silu_conv2d(x, g1, b1, EPS, w1, c1b, partials=True, in_part=f.part, form=ops.FORM_VAE)
        self.tap("gn_conv", name + ".conv1", dict(x=x, in_part=f.part), dict(gamma=g1, beta=b1, eps=EPS, w=self.oihw(name + ".conv1.weight"), b=c1b), h1, part=p1)
        skip = x
        if (name + ".nin_shortcut.weight") in self.shapes:
            wn, bn = self.mat(name + ".nin_shortcut.weight"), self.vec(name + ".nin_shortcut.bias")
            skip = ops.conv2d(x, wn, bn, ksize=1, form=ops.FORM_VAE)
            self.tap("conv", name + ".nin_shortcut", dict(x=x), dict(w=self.oihw(name + ".nin_shortcut.weight"), b=bn), skip)
        out, po = ops.group_norm_silu_conv2d(h1, g2, b2, EPS, w2, c2b, residual=skip, partials=True, in_part=p1, form=ops.FORM_VAE)
        self.tap("gn_conv", name + ".conv2", dict(x=h1, in_part=p1, residual=skip), dict(gamma=g2, beta=b2, eps=EPS, w=self.oihw(name + ".conv2.weight"), b=c2b),
                 out, part=po)
        return Feat(out, po)

    # -- AttnBlock.forward (LD.py:3630-3642): one head of C channels (pytorch_attention, LD.py:3591-3602)
    def attn(self, name, f: Feat) -> Feat:
        ops = self.ops
        x = f.t
        n, H, Wd, C = x.shape
        L = H * Wd
        ng, nb = self.vec(name + ".norm.weight"), self.vec(name + ".norm.bias")
        g = ops.group_norm(x, ng, nb, EPS)                                 # (its own statistics pass, whatever x carries)
        self.tap("groupnorm", name + ".norm", dict(x=x, in_part=None), dict(gamma=ng, beta=nb, eps=EPS, silu=False), g)
        g2d = g.reshape(n * L, C)
        wq, wk, wv = (self.mat(f"{name}.{t}.weight") for t in "qkv")
        bq, bk, bv = (self.vec(f"{name}.{t}.bias") for t in "qkv")
        if C in (512, 256):
            wqkv = self._cached(("qkv", name), lambda: (torch.cat([wq, wk, wv]).contiguous(), torch.cat([bq, bk, bv]).contiguous()))
            qkv = ops.linear(g2d, *wqkv)
            self.tap("linear", name + ".qkv", dict(x=g2d), dict(w=wqkv[0], b=wqkv[1], act="none"), qkv)
            q3 = qkv.view(n, L, 3 * C)
            o = ops.attention_qkv(q3, 1)
            self.tap("attention", name + ".attention", dict(q=q3[..., :C], k=q3[..., C:2 * C], v=q3[..., 2 * C:]), {}, o)
        else:
            wqk = self._cached(("qk", name), lambda: (torch.cat([wq, wk]).contiguous(), torch.cat([bq, bk]).contiguous()))
            qk = ops.linear(g2d, *wqk)
            self.tap("linear", name + ".qk", dict(x=g2d), dict(w=wqk[0], b=wqk[1], act="none"), qk)
            Lp = (L + 7) // 8 * 8                                          # keys padded to 16-byte rows
            # V^T[b] = Wv g_b^T + bv, the bias along the rows
            vt = ops.linear_batched(wv, g, C, Lp, C, n, (0, L * C), lda=C, ldw=C, bias_m=bv, n_valid=L)
            self.tap("linear_batched", name + ".v^T", dict(x=wv.unsqueeze(0).expand(n, C, C), w=g.view(n, L, C)), dict(bias_m=bv, n_valid=L, alpha=1.0), vt)
            # S_b = Q_b K_b^T / sqrt(C)
            alpha = 1.0 / math.sqrt(C)
            q3 = qk.view(n, L, 2 * C)
            s = ops.linear_batched(qk, q3[..., C:], L, Lp, C, n, (L * 2 * C, L * 2 * C), lda=2 * C, ldw=2 * C, n_valid=L, alpha=alpha)
            s_raw = s.clone()                                              # (the softmax runs in place: the scores' tap keeps a copy)
            self.tap("linear_batched", name + ".qk^T", dict(x=q3[..., :C], w=q3[..., C:]), dict(bias_m=None, n_valid=L, alpha=alpha), s_raw)
            p = ops.softmax_rows_ld_(s.view(n * L, Lp), Lp, L).view(n, L, Lp)
            self.tap("softmax", name + ".softmax", dict(s=s_raw), dict(valid=L), p)
            o = ops.linear_batched(p, vt, L, C, Lp, n, (L * Lp, C * Lp), lda=Lp, ldw=Lp)
            self.tap("pv", name + ".pv", dict(p=p, vt=vt), dict(valid=L), o)
        wo, bo = self.mat(name + ".proj_out.weight"), self.vec(name + ".proj_out.bias")
        o2d, x2d = o.reshape(n * L, C), x.reshape(n * L, C)
        out = ops.linear(o2d, wo, bo, residual=x2d)
        self.tap("linear", name + ".proj_out", dict(x=o2d, residual=x2d), dict(w=wo, b=bo, act="none"), out)
        return Feat(out.view(n, H, Wd, C))

    def norm_out(self, name, f: Feat):
        ops = self.ops
        og, ob = self.vec(name + ".weight"), self.vec(name + ".bias")
        if f.part is not None:
            g = ops.group_norm_from_partials(f.t, f.part, og, ob, EPS, silu=True)
        else:
            g = ops.group_norm(f.t, og, ob, EPS, silu=True)
        return self.tap("groupnorm", name, dict(x=f.t, in_part=f.part), dict(gamma=og, beta=ob, eps=EPS, silu=True), g)

    def _walk(self, mods, f: Feat) -> Feat:
        """The res / attn / up / down modules between conv_in and norm_out."""
        ops = self.ops
        for kind, name, cin, cout in mods:
            if kind == "res":
                f = self.resblock(name, f)
            elif kind == "attn":
                f = self.attn(name, f)
            elif kind == "up":              # Upsample: nearest 2x, then the convolution (its loader reads the source at half the coordinates)
                wu, bu = self.conv3(name + ".weight"), self.vec(name + ".bias")
                hv, wv = 2 * f.t.shape[1], 2 * f.t.shape[2]
                out, po = ops.conv2d_gn_partials(f.t, wu, bu, out_hw=(hv, wv), form=ops.FORM_VAE)
                self.tap("conv", name, dict(x=f.t, out_hw=(hv, wv)), dict(w=self.oihw(name + ".weight"), b=bu), out, part=po)
                f = Feat(out, po)
            elif kind == "down":            # Downsample: F.pad (0, 1, 0, 1), then the 3x3 stride-2 convolution without padding
                wd, bd = self.conv3(name + ".weight"), self.vec(name + ".bias")
                out = ops.conv2d(f.t, wd, bd, stride=2, pad=0, form=ops.FORM_VAE)
                self.tap("conv", name, dict(x=f.t, stride=2, pad=(0, 1, 0, 1)), dict(w=self.oihw(name + ".weight"), b=bd), out)
                f = Feat(out)
        return f

    # -- post_quant_conv, Decoder.forward, VAE.decode's clamp((x + 1) / 2) and NHWC output
    def decode(self, z: torch.Tensor) -> torch.Tensor:
        """z [n][4][h][w] fp32 -> image [n][8h][8w][out_ch] fp32 in [0, 1] on the device."""
        ops, cfg = self.ops, self.cfg
        self.taps = []
        z = z.to(self.dev, torch.float32).contiguous()
        mods = modules(cfg)
        wi, bi = self.conv3("decoder.conv_in.weight"), self.vec("decoder.conv_in.bias")
        pw, pb = self.mat("post_quant_conv.weight"), self.vec("post_quant_conv.bias")
        y = ops.small_conv_in(z, wi, bi, pre_w=pw, pre_b=pb)
        self.tap("conv_in", "post_quant_conv>decoder.conv_in", dict(x=z), dict(w=wi, b=bi, pre_w=pw, pre_b=pb), y)
        f = self._walk(mods[1:-2], Feat(y))
        g = self.norm_out("decoder.norm_out", f)
        n, H, Wd, C = g.shape
        oc = cfg["out_ch"]
        wo, bo = self.conv3("decoder.conv_out.weight"), self.vec("decoder.conv_out.bias")
        if ops.vae_conv_out_takes_halo_tile(C, n, H, Wd, oc):
            # the weights zero-padded to 32 rows, 8 stored columns, then the clamp as an element-wise pass
            wp, bp = self._cached(("co_pad", C), lambda: self._padded(wo, bo))
            t8 = ops.conv2d(g, wp, bp, n_valid=8, ldc=8, form=ops.FORM_VAE)
            self.tap("conv_pad", "decoder.conv_out", dict(x=g), dict(w=self.oihw("decoder.conv_out.weight"), b=bo), t8)
            out = ops.vae_out_finish(t8, oc)
            self.tap("out_finish", "decoder.conv_out (clamp)", dict(t8=t8), dict(cout=oc), out)
            return out.view(n, H, Wd, oc)
        out = ops.small_conv_out(g, wo, bo, 1)
        return self.tap("conv_out", "decoder.conv_out", dict(x=g), dict(w=wo, b=bo, mode=1), out)

    @staticmethod
    def _padded(wo, bo):
        wp = torch.zeros(32, wo.shape[1], dtype=torch.float16, device=wo.device)
        bp = torch.zeros(32, dtype=torch.float16, device=wo.device)
        wp[:wo.shape[0]] = wo
        bp[:bo.shape[0]] = bo
        return wp, bp

    # -- VAE.encode's device part: process_input, Encoder.forward, quant_conv
    def encode_moments(self, pixels: torch.Tensor) -> torch.Tensor:
        """pixels [n][H][W][3] in [0, 1] -> moments [n][2z][H/8][W/8] fp32 (mean | logvar) on the device."""
        assert self.with_encoder
        ops, cfg = self.ops, self.cfg
        self.taps = []
        px = pixels[..., :3].to(self.dev, torch.float32).movedim(-1, 1)
        px = (px * 2.0 - 1.0).contiguous()                                   # process_input, LD.py:6295
        mods = modules(cfg, encoder=True)
        wi, bi = self.conv3("encoder.conv_in.weight"), self.vec("encoder.conv_in.bias")
        y = ops.small_conv_in(px, wi, bi)
        self.tap("conv_in", "encoder.conv_in", dict(x=px), dict(w=wi, b=bi, pre_w=None, pre_b=None), y)
        f = self._walk(mods[1:-3], Feat(y))
        g = self.norm_out("encoder.norm_out", f)
        n, H, Wd, C = g.shape
        wo, bo = self.conv3("encoder.conv_out.weight"), self.vec("encoder.conv_out.bias")
        m = ops.conv2d(g, wo, bo, form=ops.FORM_VAE)
        self.tap("conv", "encoder.conv_out", dict(x=g), dict(w=self.oihw("encoder.conv_out.weight"), b=bo), m)
        wq, bq = self.mat("quant_conv.weight"), self.vec("quant_conv.bias")
        m3 = m.view(n, H * Wd, m.shape[-1])
        out = ops.small_pointwise(m3, wq, bq)
        self.tap("quant", "quant_conv", dict(x=m3), dict(w=wq, b=bq), out)
        return out.view(n, -1, H, Wd)
