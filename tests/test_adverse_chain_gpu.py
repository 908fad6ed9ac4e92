"""The UNet and VAE executors against their operator chains on the ADVERSE network (tests/adverse.py): the same B1 / B2 / B3 code as
tests/test_unet_chain_gpu.py and tests/test_vae_chain_gpu.py (their Side classes and stage references, parametrised by the weight source), on a
network whose residual stream reaches 2^13 .. 2^15, has outlier channels, norm gains from 0.04 to 20 and SiLU / GELU arguments in the tails.

Held per case: the launch list equal entry by entry; torch.equal(executor, chain), also after every other adverse case of the handle (A, B, A);
every tap on all rows inside the existing bounds with the signed-bias statistic; the producers' partials (inside the stage references); no tap
output non-finite; and the window — the largest |fp64 stage reference| over all taps lies in [2^13, 2^15.5] (asserted on the references, not on
the device's outputs).  ESRGAN and TAESD have no normalisation and homogeneous activations: out of scope; the text model on its adverse network: tests/test_clip_chain_gpu.py.

Recorded, not asserted (tiny configs): rel-L2 and max-abs of the chain against the fp32 oracle on the same fp16-rounded weights — no derived
bound exists for a 40-layer fp16 network at these statistics.  With LD_WRITE_PARITY=1 the records go to profiles/adverse_parity.json.
"""
import json

import pytest
import torch

import adverse as A
import chain_harness as H
import errbound as EB
import test_unet_chain_gpu as TU
import test_vae_chain_gpu as TV
from conftest import rel_l2
from lightdiffusion_amd import weights as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WINDOW = (2.0 ** 13, 2.0 ** 15.5)

GAINS = A.CHAIN_GAIN          # one gain per (model, config): see tests/adverse.py

# name -> (config, nb, (h, w), tokens, mode, sigmas)
UNET_CASES = {
    "tiny_2_8x12": ("tiny", 2, (8, 12), 77, "forward", (2.5, 0.7)),
    "tiny_pair1_8x8_hi": ("tiny", 1, (8, 8), 77, "pair", (14.6,)),           # the CFG pair of one at both ends of the schedule
    "tiny_pair1_8x8_lo": ("tiny", 1, (8, 8), 77, "pair", (0.03,)),
    "sd15_pair1_16x16": ("sd15", 1, (16, 16), 77, "pair", (2.5,)),
}
VAE_CASES = {k: TV.CASES[k] for k in ("tiny_dec_1_5x7", "tiny_enc_2_3x5", "fb_dec_1_5x7", "sd15_dec_1_48x32", "sd15_enc_2_48x32")}


def unet_inputs(name):
    tag, nb, (h, w), tokens, mode, sigmas = UNET_CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    x = (torch.randn(nb, 4, h, w, generator=g) * 3.0).to(DEV)
    ctx = torch.randn(2 * nb if mode == "pair" else nb, tokens, TU.config(tag)["context_dim"], generator=g).to(DEV)
    return x, torch.tensor(sigmas, dtype=torch.float32, device=DEV), ctx


def _side(model, tag):
    src = A.source(model, gain=GAINS[(model, tag)])
    if model == "unet":
        return TU.Side(tag, source=src, cases={k: v[:5] for k, v in UNET_CASES.items()}, inputs_of=unet_inputs)
    return TV.Side(tag, source=src, cases=VAE_CASES)


side = H.side_fixture(_side)


ALL = [("unet", n) for n in UNET_CASES] + [("vae", n) for n in VAE_CASES]


def _tag(model, name):
    return (UNET_CASES if model == "unet" else VAE_CASES)[name][0]


# ------------------------------------------------------------------ B1

@pytest.mark.parametrize("model,name", ALL)
def test_same_launches(side, model, name):
    s = side(model, _tag(model, name))
    _, taps = s.chain_run(name)
    H.same_launches(name, taps, s.executor_table(name))


# ------------------------------------------------------------------ B2

@pytest.mark.parametrize("model,name", ALL)
def test_same_bits(side, model, name):
    tag = _tag(model, name)
    s = side(model, tag)
    want, _ = s.chain_run(name)
    others = [o for o in (UNET_CASES if model == "unet" else VAE_CASES) if o != name and _tag(model, o) == tag]
    H.same_bits(name, want, s.executor_run, others)                          # shape history A, B, A on the adverse handle


# ------------------------------------------------------------------ B3 and the window

@pytest.mark.parametrize("model,name", ALL)
def test_every_stage_elementwise_in_the_window(side, model, name, monkeypatch):
    s = side(model, _tag(model, name))
    out, taps = s.chain_run(name)
    peak = {"ref": 0.0, "at": "", "nonfinite": []}
    check = EB.check

    def watched(y, ref, bound, what, **kw):                                  # every stage reference passes through EB.check: record its peak
        m = float(ref.double().abs().max())
        if m > peak["ref"]:
            peak["ref"], peak["at"] = m, what
        if not bool(torch.isfinite(y.float()).all()):
            peak["nonfinite"].append(what)
        return check(y, ref, bound, what, **kw)
    monkeypatch.setattr(EB, "check", watched)
    rec, fails = H.every_stage(name, taps, (lambda tap, what: TU._stage(tap, s.chain, what)) if model == "unet" else TV._stage)
    print(f"ADVERSE CHAIN {model} {name}: peak |fp64 stage reference| {peak['ref']:.4g} at {peak['at']}; " + json.dumps(rec))
    A.record(f"chain {model} {name}", {"stages": rec, "peak_stage_reference": round(peak["ref"], 1), "peak_at": peak["at"]})
    assert not peak["nonfinite"], f"non-finite tap outputs: {peak['nonfinite'][:6]}"
    H.stages_held(fails, taps)
    assert WINDOW[0] <= peak["ref"] <= WINDOW[1], f"{name}: the largest stage reference {peak['ref']:.4g} ({peak['at']}) is outside [2^13, 2^15.5]"


# ------------------------------------------------------------------ recorded, not asserted: the chain against the fp32 oracle (tiny configs)

@pytest.mark.parametrize("model,name", [(m, n) for m, n in ALL if _tag(m, n) == "tiny"])
def test_record_distance_to_the_fp32_oracle(side, model, name):
    from oracle import sd15_ref as O
    s = side(model, "tiny")
    out, _ = s.chain_run(name)
    if model == "unet":
        _, nb, _, _, mode, _ = UNET_CASES[name]
        x, sigma, ctx = unet_inputs(name)
        sd = A.state_dict("unet", W.unet_param_shapes(s.cfg), gain=GAINS[("unet", "tiny")])
        if mode == "pair":
            x, sigma = torch.cat([x, x]), torch.cat([sigma, sigma])
        ref = O.apply_model(sd, s.cfg, O.ModelSampling(), x.cpu(), sigma.cpu(), ctx.cpu())
    else:
        x = TV.inputs(name).cpu()
        if VAE_CASES[name][1] == "decode":
            ref = O.vae_decode(A.state_dict("vae", W.vae_decoder_param_shapes(s.cfg)), s.cfg, x)
        else:
            ref = O.vae_encode_moments(A.state_dict("vae", W.vae_encoder_param_shapes(s.cfg)), s.cfg, x)
    got = out.float().cpu()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all())
    rl2, mx = rel_l2(got, ref), float((got - ref).abs().max())
    print(f"ADVERSE ORACLE {model} {name}: rel-L2 {rl2:.3e}, max-abs {mx:.3e} (output max {float(ref.abs().max()):.3g})")
    A.record(f"chain {model} {name}", {"rel_l2_vs_fp32_oracle": float(f"{rl2:.4g}"), "max_abs_vs_fp32_oracle": float(f"{mx:.4g}")})
