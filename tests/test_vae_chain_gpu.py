"""The VAE executor (csrc/vae.hip run_decode / run_encode) against a chain of operator calls (tests/vae_chain.py), per launch and per bit; every
stage of the chain element-wise against fp64 on the operands the network really feeds it.

B1  same launches: the chain's launch list (ops.last_launches() of every call) equals the executor's launch table (profile_launches after
    profile_decode / profile_encode), entry by entry; a mismatch names the first differing layer.  REACHES: what each case is in the table for.
B2  same bits: torch.equal(executor, chain) on decode_device / encode_moments for every case — also with every other case of the config run in
    between on the same handle (decode, encode, decode: arena reuse, the decode plan cache that an encode drops, the padded output weights
    refilled per run).  No tolerance.  Layers held under an exception instead: none.
B3  every stage element-wise: for each tap the fp64 reference of that one stage from the stage's own fp16 inputs, the bound of tests/errbound.py
    and EB.check with the signed-bias statistic (EB.rtn_noise on top below 10^4 elements: chain_harness.held), producer partials
    against fp64 sums of the stored outputs.  What only the VAE has: the statistics handed from a halo tile's epilogue to the next GroupNorm
    (tile partials; from 192 tiles on), the encoder's stride-2 convolution with zeros below and right of the image only, the three batched
    GEMMs around the row softmax with keys padded to a multiple of 8 (the pad columns of V^T and of the scores repeat the last valid column —
    errbound.linear_batched_ref — and P's are exactly zero), the output convolution on weights padded to 32 rows with 8 stored columns (columns
    out_ch .. 7 exactly zero), post_quant_conv folded into conv_in, quant_conv.
    Every stage is held on ALL of its rows: the full fp64 im2col of the two largest resolutions (2 x 384 x 256 pixels x 1152 columns, per
    image) fits the device and takes well under a second per stage; no stage uses the row subset.
    With LD_WRITE_PARITY=1 the worst error / bound and signed bias per stage kind and case go to profiles/vae_chain_parity.json (a record).
B4  the chain is the reference's network: its output on the vae_tiny / vae_enc_tiny goldens meets the bounds of tests/test_models_gpu.py, and
    one decode case the oracle's vae_decode.

Cases (latent sizes; an encode case's image is 8x as large): the smallest that reach each path, as the issue lists them.  All named shapes
reach what they are listed for (REACHES asserts it).
"""
import json

import pytest
import torch

import chain_harness as H
import errbound as EB
from conftest import load_golden, rel_l2
from lightdiffusion_amd import weights as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FALLBACK = dict(z_channels=4, ch=64, ch_mult=[1, 1, 1, 1], num_res_blocks=2, out_ch=3)      # mid width 64: no flash kernel (test_configs_gpu.py)

# name -> (config, "decode" | "encode", (n, h, w) of the latent)
CASES = {
    "tiny_dec_1_5x7": ("tiny", "decode", (1, 5, 7)),            # 35 keys: the masked last key tile; non-square
    "tiny_dec_3_3x3": ("tiny", "decode", (3, 3, 3)),            # odd batch, 9 keys
    "tiny_dec_2_8x6": ("tiny", "decode", (2, 8, 6)),
    "tiny_enc_1_8x6": ("tiny", "encode", (1, 8, 6)),            # stride 2 at every level, even sizes: the last row and column read the zeros
    "tiny_enc_2_3x5": ("tiny", "encode", (2, 3, 5)),            # 15 keys
    "fb_dec_1_5x7": ("fallback", "decode", (1, 5, 7)),          # Lp = 40 > L = 35
    "fb_dec_2_3x3": ("fallback", "decode", (2, 3, 3)),          # Lp = 16 > L = 9, a batch stride
    "fb_enc_1_8x8": ("fallback", "encode", (1, 8, 8)),          # Lp = L = 64
    "sd15_dec_2_48x32": ("sd15", "decode", (2, 48, 32)),        # the four halo instantiations, handed-over statistics, the padded output convolution
    "sd15_dec_1_48x32": ("sd15", "decode", (1, 48, 32)),        # half the tiles: handed-over and recomputed statistics alternate
    "sd15_enc_2_48x32": ("sd15", "encode", (2, 48, 32)),        # fused routes and the handover on the encoder side
}


def config(tag):
    return {"tiny": W.tiny_vae_config(), "sd15": W.sd15_vae_config(), "fallback": FALLBACK}[tag]


def inputs(name):
    tag, mode, (n, h, w) = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    if mode == "decode":
        return (torch.randn(n, 4, h, w, generator=g) * (0.2 / 0.18215 if tag == "sd15" else 1.0)).to(DEV)
    return torch.rand(n, 8 * h, 8 * w, 3, generator=g).to(DEV)


class Side:
    """One config and weight source: the executor's handle, the chain, and per case the chain's output and taps (computed once, never changed).
    source: a WeightSource for both (None: the synthetic checkpoint); cases: another case table with CASES' names (None: CASES)."""

    def __init__(self, tag, source=None, cases=None):
        from lightdiffusion_amd.unet import MI355XVAE, synthetic_vae
        from vae_chain import VAEChain
        self.tag, self.cfg = tag, config(tag)
        self.cases = CASES if cases is None else cases
        mine = [c[2] for c in self.cases.values() if c[0] == tag]
        kw = dict(max_batch=max(s[0] for s in mine), max_hw=(max(s[1] for s in mine), max(s[2] for s in mine)), with_encoder=True)
        self.vae = synthetic_vae(self.cfg, **kw) if source is None else MI355XVAE(self.cfg, source, **kw)
        self.chain = VAEChain(self.cfg, DEV, with_encoder=True, source=source)
        self._chain_runs = {}

    def chain_run(self, name):
        if name not in self._chain_runs:
            x = inputs(name)
            out = self.chain.decode(x) if self.cases[name][1] == "decode" else self.chain.encode_moments(x)
            self._chain_runs[name] = (out, self.chain.taps)
        return self._chain_runs[name]

    def executor_run(self, name):
        x = inputs(name)
        return self.vae.decode_device(x) if self.cases[name][1] == "decode" else self.vae.encode_moments(x)

    def executor_table(self, name):
        x = inputs(name)
        rows = self.vae.profile_decode(x) if self.cases[name][1] == "decode" else self.vae.profile_encode(x)
        return [r[4] for r in rows]


side = H.side_fixture(Side)


# ------------------------------------------------------------------ B1

# kernel-name prefixes and layer-name suffixes a case must reach (a tuple: any one of them) and must NOT reach.  "gn_apply_kernel" /
# "gn_finalize_kernel" on their own: a GroupNorm that ran on a producer's statistics; "gn_stats_kernel+...": one that ran its own pass.
_OWN_STATS = ("gn_stats_kernel+gn_apply_kernel", "gn_stats_kernel+gn_finalize_kernel")
_HANDED = ("gn_apply_kernel", "gn_finalize_kernel")
_TINY_DEC = ("small_conv_in_kernel", "small_conv_out_kernel", "flash_attn512_kernel<256,masked>", "gn_stats_kernel+gn_apply_kernel", ".nin_shortcut", ".upsample.conv")
_TINY_ENC = ("small_conv_in_kernel", "small_pointwise_kernel", "flash_attn512_kernel<256,masked>", "gn_stats_kernel+gn_apply_kernel", ".nin_shortcut", ".downsample.conv")
_FB = ("softmax_rows_kernel", ".v^T", ".qk^T", ".pv", "gn_stats_kernel+gn_apply_kernel")
REACHES = {
    "tiny_dec_1_5x7": _TINY_DEC, "tiny_dec_3_3x3": _TINY_DEC, "tiny_dec_2_8x6": _TINY_DEC,
    "tiny_enc_1_8x6": _TINY_ENC, "tiny_enc_2_3x5": _TINY_ENC,
    "fb_dec_1_5x7": _FB + ("small_conv_out_kernel",), "fb_dec_2_3x3": _FB + ("small_conv_out_kernel",), "fb_enc_1_8x8": _FB + ("small_pointwise_kernel", ".downsample.conv"),
    "sd15_dec_2_48x32": ("conv6_kernel<W128,halo+groupnorm,128x512>", "conv6_kernel<W128,halo,256,up>", "conv6_kernel<W128,halo+groupnorm,256>",
                         "conv6_kernel<W128,halo,32x512>", "vae_out_finish_kernel", "flash_attn512_kernel<512", "gn_finalize_kernel", _HANDED, ".nin_shortcut"),
    "sd15_dec_1_48x32": ("flash_attn512_kernel<512", _OWN_STATS, _HANDED, "conv6_kernel<W128,halo+groupnorm"),
    "sd15_enc_2_48x32": ("conv6_kernel<W128,halo+groupnorm,128x512>", "flash_attn512_kernel<512", _HANDED, ".downsample.conv", "small_pointwise_kernel"),
}
# no statistics handover anywhere at the small shapes: every producer reported 0 chunks
NEVER = {name: _HANDED + ("conv6_kernel",) for name in CASES if not name.startswith("sd15")}


@pytest.mark.parametrize("name", list(CASES))
def test_same_launches(side, name):
    s = side(CASES[name][0])
    _, taps = s.chain_run(name)
    mine = H.same_launches(name, taps, s.executor_table(name))
    names = {k for _, k in mine}
    layers = [t["name"] for t in taps]
    print(f"LAUNCHES {name}: {sorted(names)}")
    reached = lambda want: any(k.startswith(want) for k in names) or any(l.endswith(want) for l in layers)
    for want in REACHES[name]:
        alts = want if isinstance(want, tuple) else (want,)
        assert any(reached(w) for w in alts), f"{name} no longer reaches {' or '.join(alts)}: {sorted(names)}"
    for bad in NEVER.get(name, ()):
        assert not any(k.startswith(bad) for k in names), f"{name} was to run without {bad}: {sorted(names)}"
    handed = [t["name"] for t in taps if t["inp"].get("in_part") is not None]
    assert bool(handed) == name.startswith("sd15"), (name, handed)
    if CASES[name][0] == "fallback":                        # the padded key axis the case is listed for
        sm = next(t for t in taps if t["kind"] == "softmax")
        n, h, w = CASES[name][2]
        assert sm["par"]["valid"] == h * w and sm["out"].shape == (n, h * w, (h * w + 7) // 8 * 8)
    if name == "sd15_dec_1_48x32":                          # both kinds of GroupNorm in one run, in the ResnetBlocks themselves
        gn = [t["inp"]["in_part"] is not None for t in taps if t["kind"] == "gn_conv"]
        assert any(gn) and not all(gn), gn


# ------------------------------------------------------------------ B2

@pytest.mark.parametrize("name", list(CASES))
def test_same_bits(side, name):
    tag = CASES[name][0]
    s = side(tag)
    want, _ = s.chain_run(name)
    # shape history A, B, A — decodes and encodes on the one handle
    H.same_bits(name, want, s.executor_run, [o for o in CASES if o != name and CASES[o][0] == tag])


# ------------------------------------------------------------------ B3

def _per_image(fn, n):
    """A stage reference image by image (the fp64 im2col of one 384 x 256 image is 0.9 GB): fn(i) -> (ref, bound) of image i, concatenated."""
    parts = [fn(i) for i in range(n)]
    return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])


def _stage(tap, what):
    """[(error / bound, signed bias)] of one tap's output(s) against the fp64 reference of that stage."""
    kind, i, p, out = tap["kind"], tap["inp"], tap["par"], tap["out"]
    if kind == "conv_in":
        ref, bound = EB.small_conv_in_ref(i["x"], p["w"], p["b"], pre_w=p["pre_w"], pre_b=p["pre_b"])
        return [H.held(out.reshape(ref.shape), ref, bound, what)]
    if kind == "conv_out":
        ref, bound = EB.small_conv_out_ref(i["x"], p["w"], p["b"], p["mode"])
        return [H.held(out.reshape(ref.shape), ref, bound, what)]
    if kind == "groupnorm":
        ref, bound = EB.groupnorm_ref(i["x"], None, p["gamma"], p["beta"], p["eps"], p["silu"])
        return [H.held(out.reshape(ref.shape), ref, bound, what)]
    if kind in ("conv", "conv_pad"):
        x = i["x"]
        n, cout = x.shape[0], p["w"].shape[0]
        res = i.get("residual")
        hw = []

        def one(j):
            ref, bound, (ho, wo) = EB.conv_ref(x[j:j + 1], p["w"], p["b"], None if res is None else res[j:j + 1], i.get("stride", 1), i.get("out_hw"), pad=i.get("pad"))
            hw[:] = [ho, wo]
            return ref, bound
        ref, bound = _per_image(one, n)
        ho, wo = hw
        if tap.get("part") is not None:
            H.partials_held(tap["part"], out, what)
        got = out.reshape(-1, out.shape[-1])
        if kind == "conv_pad":                                  # 8 stored columns: the real ones, then exact zeros (zero weight rows, zero biases)
            assert bool((got[:, cout:] == 0).all()), f"{what}: the stored columns {cout} .. 7 are not zero"
            got = got[:, :cout]
        assert tuple(out.shape[1:3]) == (ho, wo), (what, out.shape, ho, wo)
        return [H.held(got, ref, bound, what, image_rows=ho * wo, width=wo)]
    if kind == "gn_conv":
        x = i["x"]
        n, h, w, _ = x.shape
        cout = p["w"].shape[0]
        res = i.get("residual")
        ref, bound = _per_image(lambda j: EB.gn_silu_conv_ref(x[j:j + 1], p["gamma"], p["beta"], p["eps"], p["w"], p["b"], residual=None if res is None else res[j:j + 1]), n)
        if tap.get("part") is not None:
            H.partials_held(tap["part"], out, what)
        return [H.held(out.reshape(-1, cout), ref, bound, what, image_rows=h * w, width=w)]
    if kind == "linear":
        ref, bound = EB.linear_ref(i["x"], p["w"], p["b"], i.get("residual"), 1.0, p["act"])
        return [H.held(out, ref, bound, what)]
    if kind == "attention":
        ref, bound = EB.attention_ref(i["q"].contiguous(), i["k"].contiguous(), i["v"].contiguous(), 1)
        return [H.held(out, ref, bound, what)]
    if kind == "linear_batched":
        nv = p["n_valid"]
        ref, bound = EB.linear_batched_ref(i["x"], i["w"], bias_m=p["bias_m"], n_valid=nv, alpha=p["alpha"])
        EB.pad_columns_held(out, nv, what)
        return [H.held(out[..., :nv], ref, bound, what)]
    if kind == "softmax":
        lp = out.shape[-1]
        ref, bound = EB.softmax_ref(i["s"].reshape(-1, lp), p["valid"])
        got = out.reshape(-1, lp)
        assert bool((got[:, p["valid"]:] == 0).all()), f"{what}: pad columns must be exactly 0"
        keep = EB.top_half_per_row(ref)
        return [H.held(got, ref, bound, what, keep=keep, bias_extra=EB.subnormal_bias_allowance(ref, keep))]
    if kind == "pv":
        ref, bound = EB.pv_ref(i["p"], i["vt"], p["valid"])
        return [H.held(out, ref, bound, what)]
    if kind == "out_finish":
        ref, bound = EB.vae_out_finish_ref(i["t8"], p["cout"])
        return [H.held(out, ref, bound, what, keep=torch.ones_like(ref, dtype=torch.bool))]
    if kind == "quant":
        ref, bound = EB.small_pointwise_ref(i["x"], p["w"], p["b"])
        return [H.held(out, ref, bound, what)]
    raise AssertionError(f"no reference for stage kind {kind}")


@pytest.mark.parametrize("name", list(CASES))
def test_every_stage_elementwise(side, name):
    s = side(CASES[name][0])
    _, taps = s.chain_run(name)
    rec, fails = H.every_stage(name, taps, _stage)
    print(f"PARITY {name}: " + json.dumps(rec))
    H.record("vae_chain_parity.json", name, rec)
    H.stages_held(fails, taps)


# ------------------------------------------------------------------ B4

def test_chain_meets_the_goldens(side):
    s = side("tiny")
    g = load_golden("vae_tiny")
    img = s.chain.decode(g["z"]).cpu()
    assert img.shape == g["img"].shape
    assert float((img - g["img"]).abs().max()) < 2.0 / 255.0 and float((img - g["img"]).abs().mean()) < 0.25 / 255.0
    g = load_golden("vae_enc_tiny")
    m = s.chain.encode_moments(g["pixels"]).cpu()
    assert m.shape == g["moments"].shape and rel_l2(m, g["moments"]) < 5e-3, rel_l2(m, g["moments"])


def test_chain_meets_the_oracle(side):
    from oracle import sd15_ref as O
    name = "tiny_dec_1_5x7"
    s = side("tiny")
    out, _ = s.chain_run(name)
    ref = O.vae_decode(W.synth_state_dict(W.vae_decoder_param_shapes(s.cfg)), s.cfg, inputs(name).cpu())
    assert out.shape == ref.shape and float((out.cpu() - ref).abs().max()) < 2.0 / 255.0, float((out.cpu() - ref).abs().max())
