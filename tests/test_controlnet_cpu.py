"""CPU: ControlNet's host side and its fp32 reference (tests/controlnet_ref.py).
  * the reference walk gives one residual per input block plus the middle one, with the skip shapes of oracle.sd15_ref.unet_plan;
  * THE CONDITION the GPU comparisons rest on: with the synthetic ControlNet at strength 1 the reference's controlled output differs from its
    uncontrolled one by rel-L2 >= 0.05 = 10 x UNET_TOL — only then can a 5e-3 comparison tell "control applied" from "control ignored";
  * weights.controlnet_param_shapes is the cldm layout, and what the loader's configuration detection reads back;
  * the node shells set the keys upstream sets; the step-range predicate holds both boundary sigmas;
  * without apply_control a conditioning that carries "control" samples exactly as one without (a stand-in model), with it the guided step gets
    the ControlNet exactly while sigma is inside its range;
  * what is out of scope raises."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import controlnet_ref as R                                                        # noqa: E402
from conftest import rel_l2                                                       # noqa: E402
from test_preview_cpu import _ToyInner, _ToyPatcher, host_update_arithmetic      # noqa: E402,F401  (the fixture is used by name)
from lightdiffusion_amd import checkpoint as CK                                   # noqa: E402
from lightdiffusion_amd import nodes as N                                         # noqa: E402
from lightdiffusion_amd import sampling as S                                      # noqa: E402
from lightdiffusion_amd import weights as W                                       # noqa: E402
from lightdiffusion_amd.controlnet import ControlNet, common_upscale             # noqa: E402
from oracle import sd15_ref as O                                                  # noqa: E402

UNET_TOL = 5e-3          # the per-call bound of tests/test_models_gpu.py
CFG = W.tiny_unet_config()


def case(b, h, w, seed=3):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(b, 4, h, w, generator=g) * 3.0
    s = torch.tensor([2.5, 0.7][:b])
    ctx = torch.randn(b, 77, CFG["context_dim"], generator=g)
    hint = torch.rand(1, 3, 8 * h, 8 * w, generator=g)
    return x, s, ctx, hint


@pytest.fixture(scope="module")
def nets():
    return W.synth_state_dict(W.unet_param_shapes(CFG)), R.synth_state_dict(CFG), O.ModelSampling()


# ------------------------------------------------------------------ the reference
@pytest.mark.parametrize("b,h,w", [(1, 16, 16), (2, 8, 24)])
def test_reference_residuals_have_the_skip_shapes_and_control_moves_the_output(nets, b, h, w):
    sd, cn, ms = nets
    x, s, ctx, hint = case(b, h, w)
    plan = O.unet_plan(CFG)
    res = R.control_residuals(cn, CFG, ms, x, s, ctx, hint)
    assert len(res) == len(plan["input"]) + 1
    # the skip shapes: walk the plan as unet_forward does
    C, H, Wd, shapes = CFG["model_channels"], h, w, []
    for layers in plan["input"]:
        for kind, p in layers:
            if kind == "res":
                C = sd[p + ".out_layers.3.weight"].shape[0]
            elif kind == "down":
                H, Wd = (H - 1) // 2 + 1, (Wd - 1) // 2 + 1
        shapes.append((b, C, H, Wd))
    shapes.append(shapes[-1])
    assert [tuple(r.shape) for r in res] == shapes
    # without control the restated walk is the oracle's, bit for bit
    plain = R.apply_model(sd, CFG, ms, x, s, ctx)
    assert torch.equal(plain, O.apply_model(sd, CFG, ms, x, s, ctx))
    # THE CONDITION: control at strength 1 moves the reference by at least 10 x UNET_TOL; strength 0 and all-zero zero convolutions do not move it
    moved = rel_l2(R.apply_model(sd, CFG, ms, x, s, ctx, cn, hint, 1.0), plain)
    assert moved >= 10 * UNET_TOL, moved
    assert torch.equal(R.apply_model(sd, CFG, ms, x, s, ctx, cn, hint, 0.0), plain)
    zeroed = {k: (torch.zeros_like(v) if k.startswith(("zero_convs.", "middle_block_out.")) else v) for k, v in cn.items()}
    assert torch.equal(R.apply_model(sd, CFG, ms, x, s, ctx, zeroed, hint, 1.0), plain)


def test_a_batch_one_hint_serves_the_batch(nets):
    _, cn, ms = nets
    x, s, ctx, hint = case(2, 8, 8)
    a = R.control_residuals(cn, CFG, ms, x, s, ctx, hint)
    b = R.control_residuals(cn, CFG, ms, x, s, ctx, hint.expand(2, -1, -1, -1))
    # (torch's fp32 convolution sums in another order at another batch: fp32 rounding, 2^-23 a term, not bits)
    assert all(rel_l2(p, q) < 1e-5 for p, q in zip(a, b))


# ------------------------------------------------------------------ shapes and the loader's detection
@pytest.mark.parametrize("cfg", [W.tiny_unet_config(), W.sd15_unet_config()])
def test_param_shapes_are_the_cldm_layout_and_detection_reads_them_back(cfg):
    shp = W.controlnet_param_shapes(cfg, hint_channels=3)
    unet = W.unet_param_shapes(cfg)
    n_in = len(O.unet_plan(cfg)["input"])
    assert not any(k.startswith(("output_blocks.", "out.")) for k in shp)
    assert all(shp[k] == unet[k] for k in unet if k.startswith(("time_embed.", "input_blocks.", "middle_block.")))
    assert sorted(int(k.split(".")[1]) for k in shp if k.startswith("zero_convs.") and k.endswith(".weight")) == list(range(n_in))
    assert [shp[f"input_hint_block.{2 * i}.weight"][:2] for i in range(8)] == \
        [(16, 3), (16, 16), (32, 16), (32, 32), (96, 32), (96, 96), (256, 96), (cfg["model_channels"], 256)]
    top = cfg["model_channels"] * cfg["channel_mult"][-1]
    assert shp["middle_block_out.0.weight"] == (top, top, 1, 1) and shp[f"zero_convs.{n_in - 1}.0.weight"] == (top, top, 1, 1)
    assert shp["zero_convs.0.0.weight"] == (cfg["model_channels"],) * 2 + (1, 1)
    for prefix in ("", "control_model."):
        sd = {prefix + k: torch.empty(s, device="meta") for k, s in shp.items()}
        got, hc = CK.detect_controlnet_config(CK.controlnet_state_dict(sd), num_heads=cfg["num_heads"])
        assert hc == 3
        for k in ("in_channels", "model_channels", "channel_mult", "num_res_blocks", "transformer_depth", "transformer_depth_middle", "context_dim"):
            assert got[k] == cfg[k], k
        assert W.controlnet_param_shapes(got, hc) == shp


def test_other_file_layouts_are_refused():
    for sd in ({"controlnet_cond_embedding.conv_in.weight": 0}, {"lora_controlnet": 0, "input_hint_block.0.weight": 0}, {"adapter.body.0.weight": 0},
               {"input_blocks.0.0.weight": 0}):
        with pytest.raises(ValueError):
            CK.controlnet_state_dict(sd)


def test_synthetic_weights_do_not_repeat_the_unets():
    s = (64, 64, 3, 3)
    assert not torch.equal(W.synth_controlnet_tensor("input_blocks.1.0.in_layers.2.weight", s), W.synth_tensor("input_blocks.1.0.in_layers.2.weight", s))


# ------------------------------------------------------------------ nodes
def conditioning(seed, **keys):
    return [[torch.randn(1, 77, 8, generator=torch.Generator().manual_seed(seed)), dict(keys)]]


def test_node_shells_set_upstreams_keys():
    cn = ControlNet(None)
    image = torch.rand(1, 16, 24, 3)
    pos = conditioning(1, pooled_output=None)
    out = N.ControlNetApply().apply_controlnet(pos, cn, image, 0.75)[0]
    d = out[0][1]
    assert out[0][0] is pos[0][0] and "control" not in pos[0][1]                  # the caller's list is not modified
    assert d["control_apply_to_uncond"] is True and isinstance(d["control"], ControlNet) and d["control"] is not cn
    assert d["control"].strength == 0.75 and d["control"].timestep_percent_range == (0.0, 1.0)
    assert tuple(d["control"].cond_hint_original.shape) == (1, 3, 16, 24)         # NCHW
    assert d["control"].control_model is cn.control_model and "pooled_output" in d
    assert N.ControlNetApply().apply_controlnet(pos, cn, image, 0)[0] is pos      # strength 0: the conditioning as it came
    neg = conditioning(2)
    p2, n2 = N.ControlNetApplyAdvanced().apply_controlnet(pos, neg, cn, image, 0.5, 0.1, 0.6)
    assert p2[0][1]["control"] is n2[0][1]["control"]                             # ONE copy on both lists
    assert p2[0][1]["control_apply_to_uncond"] is False and n2[0][1]["control_apply_to_uncond"] is False
    assert p2[0][1]["control"].timestep_percent_range == (0.1, 0.6) and p2[0][1]["control"].strength == 0.5
    assert N.ControlNetApplyAdvanced().apply_controlnet(pos, neg, cn, image, 0, 0.0, 1.0) == (pos, neg)
    with pytest.raises(NotImplementedError):                                      # a second ControlNet on the same entries: chained
        N.ControlNetApply().apply_controlnet(out, cn, image, 1.0)


def test_controlnet_object_surface():
    cn = ControlNet("model").set_cond_hint(torch.rand(1, 3, 8, 8), 0.5, (0.25, 0.75))
    c2 = cn.copy()
    assert c2.control_model == "model" and c2.strength == 0.5 and c2.timestep_percent_range == (0.25, 0.75) and c2.cond_hint_original is cn.cond_hint_original
    assert cn.get_models() == ["model"] and cn.previous_controlnet is None
    ms = S.ModelSampling()
    cn.pre_run(None, ms.percent_to_sigma)
    assert cn.timestep_range == (ms.percent_to_sigma(0.25), ms.percent_to_sigma(0.75)) and cn.ranged
    cn.cleanup()
    assert cn.timestep_range is None
    assert not ControlNet("m").ranged


def test_common_upscale_center_crop_then_nearest_exact():
    x = torch.arange(2 * 3 * 8 * 16, dtype=torch.float32).reshape(2, 3, 8, 16)
    y = common_upscale(x, 16, 16, "nearest-exact", "center")                      # the target is square: the middle 8 columns, doubled
    assert torch.equal(y, torch.nn.functional.interpolate(x[:, :, :, 4:12], size=(16, 16), mode="nearest-exact"))
    assert torch.equal(common_upscale(x, 16, 8), x)


# ------------------------------------------------------------------ the step range
def test_step_range_predicate_at_the_boundary_sigmas():
    ms = S.ModelSampling()
    start, end = ms.percent_to_sigma(0.2), ms.percent_to_sigma(0.6)
    assert start > end
    rng = (start, end)
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))
    up = lambda v: float(torch.nextafter(torch.tensor(v, dtype=torch.float32), torch.tensor(float("inf"))))
    down = lambda v: float(torch.nextafter(torch.tensor(v, dtype=torch.float32), torch.tensor(0.0)))
    assert S.control_step_active(rng, f32(start)) and S.control_step_active(rng, f32(end))       # both boundaries are inside
    assert not S.control_step_active(rng, up(start)) and not S.control_step_active(rng, down(end))
    assert S.control_step_active(rng, 0.5 * (start + end))
    assert S.control_step_active(None, 3.0)
    full = (ms.percent_to_sigma(0.0), ms.percent_to_sigma(1.0))
    assert S.control_step_active(full, float(ms.sigma_max)) and S.control_step_active(full, 0.0)


# ------------------------------------------------------------------ the sampler: inert without the keyword, gated by the range with it
class _Wrapper:
    """a stand-in for the resident UNet's guided step: the toy denoiser, + 1 where a ControlNet is handed in"""

    def __init__(self):
        self.inner, self.seen = _ToyInner(), []

    def cfg_denoise(self, x, timestep, ctx, cond_scale, token=None, use_graph=True, control=None):
        self.seen.append((float(timestep[0]), control))
        out = self.inner.apply_model(torch.cat([x, x]), torch.cat([timestep, timestep]), c_crossattn=ctx.expand(2 * x.shape[0], -1, -1) if ctx.shape[0] == 1 else ctx)
        u, c = out.chunk(2)
        return u + (c - u) * cond_scale + (0.0 if control is None else control.strength)

    def __call__(self, apply_model, params):
        return apply_model(params["input"], params["timestep"], **params["c"])


def patcher(wrapper=None):
    p = _ToyPatcher()
    if wrapper is not None:
        p.model_options = {"model_function_wrapper": wrapper}
    return p


def run(pos, neg, model, steps=4, **kw):
    return S.common_ksampler(model, 5, steps, 3.0, "euler_ancestral", "normal", pos, neg, {"samples": torch.zeros(2, 4, 3, 5)}, **kw)[0]["samples"]


def test_without_the_keyword_the_control_key_is_inert(host_update_arithmetic):
    cn = ControlNet(None).set_cond_hint(torch.rand(1, 3, 24, 40))
    pos, neg = conditioning(1), conditioning(2)
    cpos = N.ControlNetApply().apply_controlnet(pos, cn, torch.rand(1, 24, 40, 3), 1.0)[0]
    for make in (lambda: patcher(), lambda: patcher(_Wrapper())):
        base = run(pos, neg, make())
        assert torch.equal(run(cpos, neg, make()), base)
        assert torch.equal(run(cpos, neg, make(), apply_control=False), base)
        assert torch.equal(run(pos, neg, make(), apply_control=True), base)        # the keyword without a control
    w = _Wrapper()
    run(cpos, neg, patcher(w))
    assert w.seen and all(c is None for _, c in w.seen)


def test_with_the_keyword_control_reaches_exactly_the_steps_inside_the_range(host_update_arithmetic):
    cn = ControlNet(None)
    image = torch.rand(1, 24, 40, 3)
    pos, neg = conditioning(1), conditioning(2)
    w = _Wrapper()
    cpos = N.ControlNetApply().apply_controlnet(pos, cn, image, 0.5)[0]
    out = run(cpos, neg, patcher(w), apply_control=True)
    assert len(w.seen) == 4 and all(c is cpos[0][1]["control"] for _, c in w.seen)            # the uncond fill made the lists agree
    assert not torch.equal(out, run(pos, neg, patcher(_Wrapper())))
    assert cpos[0][1]["control"].timestep_range is None                                     # cleaned up after the run
    assert "control" not in neg[0][1]                                                       # on copies
    # a range: controlled while sigma[0] is inside [sigma(end), sigma(start)], ordinary after it
    p2, n2 = N.ControlNetApplyAdvanced().apply_controlnet(pos, neg, cn, image, 0.5, 0.0, 0.5)
    w = _Wrapper()
    run(p2, n2, patcher(w), apply_control=True)
    ms = S.ModelSampling()
    lo = ms.percent_to_sigma(0.5)
    assert [c is not None for _, c in w.seen] == [s >= lo for s, _ in w.seen]
    assert any(c is not None for _, c in w.seen) and any(c is None for _, c in w.seen)


def test_out_of_scope_cases_raise(host_update_arithmetic):
    cn = ControlNet(None)
    image = torch.rand(1, 24, 40, 3)
    pos, neg = conditioning(1), conditioning(2)
    cpos = N.ControlNetApply().apply_controlnet(pos, cn, image, 1.0)[0]
    w = lambda: patcher(_Wrapper())
    with pytest.raises(NotImplementedError, match="hook seam"):                             # no guided step behind the wrapper seam
        run(cpos, neg, patcher(), apply_control=True)
    p2, _ = N.ControlNetApplyAdvanced().apply_controlnet(pos, neg, cn, image, 1.0, 0.0, 1.0)
    with pytest.raises(NotImplementedError, match="SAME ControlNet"):                       # a control on the positive list only
        run(p2, neg, w(), apply_control=True)
    other = N.ControlNetApply().apply_controlnet(neg, cn, image, 1.0)[0]
    with pytest.raises(NotImplementedError, match="SAME ControlNet"):                       # different controls on the two lists
        run(cpos, other, w(), apply_control=True)
    with pytest.raises(NotImplementedError, match="apply_cond_areas"):
        run(cpos, neg, w(), apply_control=True, apply_cond_areas=True)
    chained = N.ControlNetApply().apply_controlnet(pos, cn, image, 1.0)[0]
    chained[0][1]["control"].previous_controlnet = cn
    with pytest.raises(NotImplementedError, match="chained"):
        run(chained, neg, w(), apply_control=True)
    with pytest.raises(NotImplementedError):
        cn.copy().set_previous_controlnet(cn)
    two = N.ConditioningCombine().combine(cpos, cpos)[0]
    with pytest.raises(NotImplementedError):                                                # several entries in a list
        run(two, neg, w(), apply_control=True)
    eager = w()
    eager.model_options["ld_eager_unbatched"] = True
    with pytest.raises(NotImplementedError, match="ld_eager_unbatched"):
        run(cpos, neg, eager, apply_control=True)


def test_the_detailer_still_refuses_a_control_net_wrapper():
    import inspect
    from lightdiffusion_amd import detailer
    assert "control_net_wrapper is not supported" in inspect.getsource(detailer)
