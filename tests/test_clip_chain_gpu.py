"""The CLIP text model on the HIP kernels, launch by launch (helper: tests/clip_chain.py; its CPU controls: tests/test_clip_chain_cpu.py).

`CLIPTextModelHIP._encode` calls `ops.*` from Python, so no executor test covers it, and what held it were norms over [B, 77, 768] taken behind a
final LayerNorm (rel-L2 < 5e-3): one wrong row of 77, a handful of channels, a residual rounded twice, a mask that leaks one key, a signed bias of
a few 1e-4 all pass those.  Here the operator calls of one forward are recorded and held:

  C1  the sequence: embed, nl x (LN, qkv, causal attention, out-proj + residual, LN, fc1 + quick-GELU, fc2 + residual), the final LayerNorm once
      and once more for `inter`; every operand bitwise the output it should be, every weight the model's named tensor.
  C2  every stage, every element, all rows, against the fp64 reference of that stage's own stored fp16 inputs inside the bound tests/errbound.py
      has for the operator, with the signed-bias statistic (at least half of the elements kept, EB.rtn_noise on top); the embedding exactly.
      With LD_WRITE_PARITY=1 the worst error / bound and signed bias / tolerance per stage kind and case go to profiles/clip_chain_parity.json.
  C3  bitwise, no tolerance: causality (ids behind p replaced: rows <= p of every stage unchanged — a masked key's P is exactly 0 and a row's
      softmax reference moves by its own maximum only), row independence (prompts permuted: row blocks permuted; M = 231 ends in a
      ragged tile), the layer pick, pooled = last[b, first EOS] (also with textual-inversion vectors), the weight lerp.
  C5  the 12-layer model against the fp64 composition of the stage references and against the fp32 oracle: rel-L2 < 5e-3 as before, the figures
      and the worst element recorded.
(C4, the routes: tests/test_routes_gpu.py.)

Cases: routes depend on width, so CLIP-L's width (h = 768, 12 heads of 64, ffn 3072, 77 tokens) with 2 layers at B = 1, 2 (a weighted prompt's
extra empty row), 3 (two chunks and that row: M = 231); the tiny config at B = 1 and 4; the 12 layers at B = 1.  And on the adverse text model
(tests/adverse.py source('clip'): a stress profile, not a checkpoint's statistics) the CLIP-L-width B = 2 and the tiny B = 1 case: C1, C2 at the
unchanged bounds, the window [2^13, 2^15.5] asserted on the fp64 stage references, figures to profiles/adverse_parity.json.  The distance of the
adverse chain to the fp32 oracle is recorded, not asserted: no derived bound exists for a network at these statistics (as for the UNet and VAE).
"""
import pytest
import torch

import adverse as A
import chain_harness as H
import clip_chain as C
import errbound as EB
from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WINDOW = (2.0 ** 13, 2.0 ** 15.5)
POSITIONS = (0, 31, 32, 63, 64, 75)

# name -> (config, B, adverse)
CASES = {"w2_b1": ("w2", 1, False), "w2_b2": ("w2", 2, False), "w2_b3": ("w2", 3, False), "tiny_b1": ("tiny", 1, False), "tiny_b4": ("tiny", 4, False),
         "sd15_b1": ("sd15", 1, False), "adverse_w2_b2": ("w2", 2, True), "adverse_tiny_b1": ("tiny", 1, True)}


class World:
    """Models and recorded runs, built once per module."""

    def __init__(self):
        from lightdiffusion_amd import ops
        from lightdiffusion_amd._lib import lib
        lib()
        self.ops, self.sds, self.models, self.runs = ops, {}, {}, {}

    def sd(self, tag, adverse=False):
        """fp32, fp16-rounded.  Tensors are functions of their names, so the CLIP-L-width configs share the 12-layer dict's."""
        wide = "tiny" if tag.startswith("tiny") else "sd15"
        gain = A.CHAIN_GAIN[("clip", tag)] if adverse else None
        key = (wide, gain)
        cfg = C.config(tag)
        if key not in self.sds:
            self.sds[key] = C.state_dict(C.config(wide), A.source("clip", gain=gain) if adverse else None)
        return {k: v for k, v in self.sds[key].items() if k in C.W.clip_param_shapes(cfg)}

    def model(self, tag, adverse=False):
        from lightdiffusion_amd.clip import CLIPTextModelHIP
        if (tag, adverse) not in self.models:
            self.models[(tag, adverse)] = CLIPTextModelHIP(C.config(tag), self.sd(tag, adverse), device=DEV)
        return self.models[(tag, adverse)]

    def run(self, name):
        if name not in self.runs:
            tag, B, adverse = CASES[name]
            self.runs[name] = C.run(self.ops, self.model(tag, adverse), C.prompts(B))
        return self.runs[name]


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.models.clear()
    w.runs.clear()
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ C1

@pytest.mark.parametrize("name", CASES)
def test_sequence(world, name):
    tag, B, adverse = CASES[name]
    calls, (last, inter, pooled) = world.run(name)
    tm = world.model(tag, adverse)
    C.check_sequence(calls, tm.cfg, tm.w)
    assert world.ops.layer_norm.__module__ == "lightdiffusion_amd.ops" and world.ops.layer_norm.__name__ == "layer_norm", "the recorder did not restore the operators"
    h = tm.cfg["hidden_size"]
    assert last.shape == inter.shape == (B, C.L, h) and pooled.shape == (B, h)
    calls, out = C.run(world.ops, tm, C.prompts(B), intermediate_output=None)          # without a layer pick: one final LayerNorm
    C.check_sequence(calls, tm.cfg, tm.w, intermediate_output=None)
    assert out[1] is None and torch.equal(out[0], last)


def test_sequence_after_a_lora_patch(world):
    """The fused [q|k|v] projection holds copies of q / k / v_proj: after a device LoRA merge onto one of each (in three layers) the recorded
    weights are still the model's named tensors (C1: the fused weight is cat(q, k, v) of the PATCHED tensors), every stage is inside its bound,
    and unpatching brings back the loaded model's bits in every stage."""
    tm = world.model("tiny")
    base, _ = world.run("tiny_b1")
    g = torch.Generator().manual_seed(11)
    h, f = tm.cfg["hidden_size"], tm.cfg["intermediate_size"]
    P = "text_model.encoder.layers."
    term = lambda n, k: [(torch.randn(n, 4, generator=g) * 0.3, torch.randn(4, k, generator=g) * 0.3, 0.5)]
    keys = {P + "0.self_attn.k_proj.weight": (h, h), P + "1.self_attn.v_proj.weight": (h, h), P + "2.self_attn.q_proj.weight": (h, h),
            P + "1.self_attn.out_proj.weight": (h, h), P + "0.mlp.fc1.weight": (f, h)}
    loaded = {k: tm.w[k].clone() for k in keys}
    try:
        tm.patch_weights({k: term(*s) for k, s in keys.items()})
        assert all(not torch.equal(tm.w[k], loaded[k]) for k in keys)
        calls, _ = C.run(world.ops, tm, C.prompts(1))
        C.check_sequence(calls, tm.cfg, tm.w)
        C.check_stages(calls, "tiny_b1 with a LoRA merged")
        assert not torch.equal(calls[-1]["out"], base[-1]["out"])
    finally:
        tm.unpatch_weights()
    assert all(torch.equal(tm.w[k], loaded[k]) for k in keys)
    again, _ = C.run(world.ops, tm, C.prompts(1))
    C.check_sequence(again, tm.cfg, tm.w)
    C.same_rows(base, again, "after unpatching")


@pytest.mark.parametrize("c", [64, 768])
def test_layernorm_uses_the_callers_eps(world, c):
    """The text model's LayerNorm passes eps = 1e-5 through the C ABI (C1 holds the argument).  At the model's activations (variance near 1) an
    eps of 1e-6 moves a row by 4.5e-6 of itself, which C2 sees only in the few outputs that beta nearly cancels; on rows of variance 1.5e-5 the
    two eps are 25 % apart in every element."""
    g = torch.Generator().manual_seed(c)
    x = (torch.randn(C.L, c, generator=g) * 2.0 ** -8 + 0.01).half().to(DEV)
    ga, be = (1.0 + 0.5 * torch.randn(c, generator=g)).half().to(DEV), (0.5 * torch.randn(c, generator=g)).half().to(DEV)
    for eps in (1e-6, 1e-5):
        y = world.ops.layer_norm(x, ga, be, eps)
        ref, bound = EB.layernorm_ref(x, ga, be, eps)
        C.held(y, ref, bound, f"layernorm C={c} at variance 1.5e-5, eps {eps}")
    other, _ = EB.layernorm_ref(x, ga, be, 1e-6)
    assert float(((other - ref).abs() / bound).max()) > 50.0                        # (the case tells the two apart)


# ------------------------------------------------------------------ C2 (and, on the adverse network, the window)

@pytest.mark.parametrize("name", CASES)
def test_every_stage_elementwise(world, name):
    tag, B, adverse = CASES[name]
    calls, _ = world.run(name)
    peak = {}
    worst = C.check_stages(calls, name, peak)
    rec = H.stage_record(worst)
    print(f"CLIP CHAIN {name}: peak |fp64 stage reference| {peak['ref']:.4g} at {peak['at']}; {rec}")
    H.record("clip_chain_parity.json", name, {"stages": rec, "peak_stage_reference": round(peak["ref"], 2), "peak_at": peak["at"]})
    assert not peak.get("nonfinite"), f"non-finite stage outputs: {peak['nonfinite'][:6]}"
    if adverse:
        A.record(f"chain clip {name}", {"stages": rec, "peak_stage_reference": round(peak["ref"], 1), "peak_at": peak["at"], "gain": A.CHAIN_GAIN[("clip", tag)]})
        assert WINDOW[0] <= peak["ref"] <= WINDOW[1], f"{name}: the largest stage reference {peak['ref']:.4g} ({peak['at']}) is outside [2^13, 2^15.5]"


# ------------------------------------------------------------------ C3

@pytest.mark.parametrize("p", POSITIONS)
@pytest.mark.parametrize("name", ["w2_b2", "tiny_b1"])
def test_causality_is_bitwise(world, name, p):
    """Ids behind position p replaced, B and every shape unchanged: rows <= p of every recorded stage are the same bits."""
    tag, B, adverse = CASES[name]
    calls, _ = world.run(name)
    ids = C.replace_after(C.prompts(B), p)
    assert bool((ids[:, p + 1:] != C.prompts(B)[:, p + 1:]).all()) and torch.equal(ids[:, :p + 1], C.prompts(B)[:, :p + 1])
    other, _ = C.run(world.ops, world.model(tag, adverse), ids)
    C.same_rows(calls, other, f"{name}: ids behind position {p} replaced", rows=slice(0, p + 1))
    changed = [i for i, (a, b) in enumerate(zip(calls, other)) if not torch.equal(a["out"][:, p + 1:], b["out"][:, p + 1:])]
    assert len(changed) == len(calls), "the replaced ids did not reach every stage's later rows"


@pytest.mark.parametrize("name,perm", [("w2_b3", (2, 0, 1)), ("w2_b3", (1, 2, 0)), ("tiny_b4", (3, 1, 0, 2))])
def test_row_independence_is_bitwise(world, name, perm):
    """The prompts of one call permuted: every stage's 77-row blocks are permuted, bit for bit (M = 231 ends in a ragged tile of any height)."""
    tag, B, adverse = CASES[name]
    calls, (last, inter, pooled) = world.run(name)
    perm = torch.tensor(perm)
    other, out = C.run(world.ops, world.model(tag, adverse), C.prompts(B)[perm])
    C.same_rows(calls, other, f"{name}: prompts permuted by {perm.tolist()}", perm=perm.to(DEV))
    assert torch.equal(out[0], last[perm]) and torch.equal(out[1], inter[perm]) and torch.equal(out[2], pooled[perm])


@pytest.mark.parametrize("tag,shorter", [("w2", "w1"), ("tiny", "tiny2")])
def test_layer_pick(world, tag, shorter):
    """inter = final LayerNorm of the stream recorded after layer nl - 2 = `last` of a model of the same weights with nl - 1 layers."""
    name = f"{tag}_b1"
    calls, (last, inter, pooled) = world.run(name)
    tm = world.model(tag)
    nl = tm.cfg["num_hidden_layers"]
    stream = calls[7 * (nl - 1)]["out"]                                    # fc2 + residual of layer nl - 2
    assert calls[7 * (nl - 1)]["args"]["residual"] is not None and torch.equal(calls[-1]["args"]["x"], stream)
    assert torch.equal(inter, calls[-1]["out"].float())
    assert torch.equal(inter, world.ops.layer_norm(stream, tm.w["text_model.final_layer_norm.weight"], tm.w["text_model.final_layer_norm.bias"], 1e-5).float())
    short = world.model(shorter)
    assert short.cfg["num_hidden_layers"] == nl - 1
    last1, inter1, _ = short(C.prompts(1), intermediate_output=None)
    assert inter1 is None and torch.equal(last1, inter), "inter is not the last hidden state of the model with one layer fewer"


def test_pooled_is_the_first_eos_row(world):
    tm = world.model("w2")
    for name in ("w2_b3", "w2_b1"):
        _, (last, inter, pooled) = world.run(name)
        C.check_pooled(last, pooled, C.prompts(CASES[name][1]), C.END, name)
    # two textual-inversion vectors: ids V-1 and V select the side table, EOS is remapped to V-1+E
    V, h = tm.cfg["vocab_size"], tm.cfg["hidden_size"]
    eos = V - 1 + 2
    ids = torch.full((2, C.L), eos, dtype=torch.long)
    ids[:, 0] = C.START
    ids[0, 1:6] = torch.tensor([1234, V - 1, V, 2345, 3456])
    ids[1, 1:31] = torch.arange(2000, 2030)
    extra = torch.randn(2, h, generator=torch.Generator().manual_seed(5)) * 0.5
    calls, (last, inter, pooled) = C.run(world.ops, tm, ids, extra_embeds=extra)
    assert C.first_eos(ids, eos).tolist() == [6, 31]
    C.check_pooled(last, pooled, ids, eos, "two textual-inversion vectors")
    C.check_sequence(calls, tm.cfg, tm.w)
    C.check_stages(calls, "w2 with two textual-inversion vectors")
    row = calls[0]["out"][0].float().cpu()
    pos = tm.w["text_model.embeddings.position_embedding.weight"].float().cpu()
    assert torch.equal(row[2], (extra[0] + pos[2]).half().float()) and torch.equal(row[3], (extra[1] + pos[3]).half().float())


def test_weight_lerp(world):
    """CLIP.encode_from_tokens on a weighted two-chunk prompt (B = 3 with the empty prompt's row) is the reference's (z - empty) * w + empty,
    evaluated on the CPU from the downloaded hidden states."""
    from lightdiffusion_amd.clip import CLIP
    tm = world.model("w2")
    ids = C.prompts(2, seed=3)
    g = torch.Generator().manual_seed(9)
    wts = torch.where(torch.rand(2, C.L, generator=g) < 0.4, torch.tensor(1.0), torch.tensor([0.8, 1.1, 1.21, 1.5])[torch.randint(0, 4, (2, C.L), generator=g)])
    pairs = [[(int(t), float(w)) for t, w in zip(ids[k].tolist(), wts[k].tolist())] for k in range(2)]
    cond, pooled = CLIP(tm, None, layer_idx=-2).encode_from_tokens(pairs, return_pooled=True)
    empty = torch.tensor([[C.START] + [C.END] * (C.L - 1)])
    last, inter, pl = tm(torch.cat([ids, empty]), intermediate_output=-2)
    out = inter.float().cpu()
    want = []
    for k in range(2):
        z, w = out[k:k + 1], torch.tensor([w for _, w in pairs[k]], dtype=torch.float32)[None, :, None]
        want.append(torch.where(w != 1.0, (z - out[-1:]) * w + out[-1:], z))
    want = torch.cat(want, dim=-2)
    assert cond.shape == (1, 2 * C.L, tm.cfg["hidden_size"]) and cond.device.type == "cpu"
    assert torch.equal(cond, want), f"{int((cond != want).sum())} elements differ, max {float((cond - want).abs().max()):.3g}"
    assert int((wts != 1.0).sum()) > 60 and not torch.equal(cond, torch.cat([out[0:1], out[1:2]], dim=-2))
    assert torch.equal(pooled, pl[0:1].float().cpu())


# ------------------------------------------------------------------ C5

def _end_to_end(world, name):
    from oracle import sd15_ref as O
    tag, B, adverse = CASES[name]
    _, (last, inter, pooled) = world.run(name)
    tm, ids = world.model(tag, adverse), C.prompts(B)
    sd = world.sd(tag, adverse)
    c_last, c_inter, c_pooled = C.compose({k: v.to(DEV) for k, v in sd.items()}, tm.cfg, ids.to(DEV))
    o_inter = O.clip_text_model(sd, tm.cfg, ids, layer_idx=-2)
    o_last = O.clip_text_model(sd, tm.cfg, ids, layer_idx=None)
    fig = {"rel_l2_last_vs_fp64_composition": rel_l2(last.cpu(), c_last.cpu()), "rel_l2_inter_vs_fp64_composition": rel_l2(inter.cpu(), c_inter.cpu()),
           "rel_l2_pooled_vs_fp64_composition": rel_l2(pooled.cpu(), c_pooled.cpu()),
           "rel_l2_last_vs_fp32_oracle": rel_l2(last.cpu(), o_last), "rel_l2_inter_vs_fp32_oracle": rel_l2(inter.cpu(), o_inter),
           "worst_element_error_inter": float((inter.double() - c_inter).abs().max()), "inter_max_abs": float(c_inter.abs().max()),
           "oracle_vs_composition_rel_l2": rel_l2(o_inter, c_inter.cpu())}
    fig = {k: float(f"{v:.4g}") for k, v in fig.items()}
    print(f"CLIP END TO END {name}: {fig}")
    assert bool(torch.isfinite(last).all() and torch.isfinite(inter).all() and torch.isfinite(pooled).all())
    return fig


def test_end_to_end_12_layers(world):
    fig = _end_to_end(world, "sd15_b1")
    H.record("clip_chain_parity.json", "sd15_b1", {"end_to_end": fig})
    for k, v in fig.items():
        if k.startswith("rel_l2"):
            assert v < 5e-3, (k, v)


@pytest.mark.parametrize("name", ["adverse_w2_b2", "adverse_tiny_b1"])
def test_record_adverse_distance_to_the_oracle(world, name):
    fig = _end_to_end(world, name)
    A.record(f"chain clip {name}", {"end_to_end": fig})
