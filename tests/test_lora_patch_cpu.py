"""CPU: the bookkeeping of LoRA weight patches on clones of a loaded model (`nodes.LoraLoader`, `ModelPatcher` / `CLIP`
add_patches / clone, LD.py:3297-3307, 6203-6219, 6611-6625) on stand-in models that only know their parameter names and shapes, and the key
resolution `merge_lora` and `LoraLoader` share (`checkpoint.resolve_lora`).  The merge itself is a device kernel: tests/test_lora_patch_gpu.py."""
import pathlib
import warnings

import pytest
import torch

from conftest import load_golden
from lightdiffusion_amd import weights as W


class _ShapesOnly:
    """stand-in for a resident UNet / text model: parameter names and shapes, and a record of what was swapped in"""

    def __init__(self, shapes):
        self._shapes = dict(shapes)
        self.applied_patches_uuid = None
        self.calls = []

    def param_shapes(self):
        return dict(self._shapes)

    def patch_weights(self, patches, uuid=None):
        self.calls.append(("patch", {k: [(tuple(u.shape), tuple(d.shape), s) for u, d, s in v] for k, v in patches.items()}))
        self.applied_patches_uuid = uuid

    def unpatch_weights(self, uuid=None):
        self.calls.append(("unpatch", None))
        self.applied_patches_uuid = uuid


def _lora(g):
    return {k[len("lora::"):]: v for k, v in g.items() if k.startswith("lora::")}


def _stand_ins():
    from lightdiffusion_amd import nodes
    from lightdiffusion_amd.clip import CLIP
    ucfg, ccfg = W.tiny_unet_config(), W.tiny_clip_config()
    unet, text = _ShapesOnly(W.unet_param_shapes(ucfg)), _ShapesOnly(W.clip_param_shapes(ccfg))
    return nodes.ModelPatcher(nodes.SD15Model(unet), "cpu"), CLIP(text), unet, text


def _golden_key_sets(g):
    unet = {"model." + str(k) for k in g["patched_unet_keys"]}
    clip = {"cond_stage_model.transformer." + str(k)[len("clip_l.transformer."):] for k in g["patched_clip_keys"]}
    return unet, clip


def test_lora_loader_bookkeeping_on_stand_in_models():
    from lightdiffusion_amd import nodes
    assert hasattr(nodes, "LoraLoader")
    g = load_golden("lora_tiny")
    lora = _lora(g)
    want_unet, want_clip = _golden_key_sets(g)
    model, clip, unet, text = _stand_ins()
    assert model.patches == {} and model.patches_uuid is None and clip.patches == {} and clip.patches_uuid is None

    # add_patches returns the matched keys (and only keys this model has)
    from lightdiffusion_amd import checkpoint as CK
    keys = {k: torch.empty(s, device="meta") for k, s in {**model.model_key_shapes(), **clip.model_key_shapes()}.items()}
    resolved = CK.resolve_lora(keys, lora)
    probe = model.clone()
    assert set(probe.add_patches(resolved, 0.8)) == want_unet
    assert set(clip.clone().add_patches(resolved, 0.6)) == want_clip
    assert model.patches == {} and model.patches_uuid is None               # the probe clone did not touch the original

    with warnings.catch_warnings(record=True) as wl:
        warnings.simplefilter("always")
        m1, c1 = nodes.LoraLoader().load_lora(model, clip, lora, 0.8, 0.6)
    assert any("match no layer" in str(w.message) and "lora_unet_not_a_layer_of_this_model" in str(w.message) for w in wl)
    assert set(m1.patches) == want_unet and set(c1.patches) == want_clip
    assert m1.patches_uuid is not None and c1.patches_uuid is not None
    assert all(len(v) == 1 and v[0][0] == 0.8 for v in m1.patches.values()) and all(v[0][0] == 0.6 for v in c1.patches.values())
    # clone() isolates the patch lists
    assert model.patches == {} and model.patches_uuid is None and clip.patches == {} and clip.patches_uuid is None
    uuid1, snapshot = m1.patches_uuid, {k: list(v) for k, v in m1.patches.items()}
    # a second LoRA on the returned clones stacks: a second term on the same key
    m2, c2 = nodes.LoraLoader().load_lora(m1, c1, {k: v * 0.5 for k, v in lora.items() if "not_a_layer" not in k}, 0.3, 0.2)
    assert m1.patches_uuid == uuid1 and m1.patches == snapshot
    assert set(m2.patches) == want_unet and all(len(v) == 2 and v[0][0] == 0.8 and v[1][0] == 0.3 for v in m2.patches.values())
    assert all(len(v) == 2 for v in c2.patches.values()) and m2.patches_uuid not in (None, uuid1)
    assert m2.clone().patches_uuid == m2.patches_uuid and m2.clone().patches == m2.patches
    # a strength of 0 leaves that side unpatched
    m3, c3 = nodes.LoraLoader().load_lora(model, clip, {k: v for k, v in lora.items() if "not_a_layer" not in k}, 0.0, 0.6)
    assert m3.patches == {} and m3.patches_uuid is None and set(c3.patches) == want_clip

    # the lazy swap: alpha / rank folded into the scale; only when the resident identity differs; an empty set just unpatches
    assert m1.patch_model() is m1.model and unet.calls[-1][0] == "patch" and unet.applied_patches_uuid == uuid1
    terms = unet.calls[-1][1]
    q = terms["input_blocks.1.1.transformer_blocks.0.attn1.to_q.weight"]
    alpha = float(lora["lora_unet_input_blocks_1_1_transformer_blocks_0_attn1_to_q.alpha"])
    assert q == [((64, 4), (4, 64), 0.8 * alpha / 4)]
    assert terms["input_blocks.2.1.transformer_blocks.0.attn2.to_k.weight"][0][2] == 0.8        # no alpha in the file: scale = strength
    n = len(unet.calls)
    m1.patch_model()
    m1.clone().patch_model()
    assert len(unet.calls) == n                                                                 # already applied: nothing happens
    model.patch_model()
    assert unet.calls[-1][0] == "unpatch" and unet.applied_patches_uuid is None and len(unet.calls) == n + 1
    c1.patch_model()
    assert text.calls[-1][0] == "patch" and set(text.calls[-1][1]) == {k[len("cond_stage_model.transformer."):] for k in want_clip}


def test_resolver_and_merge_lora_agree_on_the_golden_key_set():
    from lightdiffusion_amd import checkpoint as CK
    from test_host_cpu import _synthetic_checkpoint
    g = load_golden("lora_tiny")
    lora = _lora(g)
    want_unet, want_clip = _golden_key_sets(g)
    sd, *_ = _synthetic_checkpoint()
    with warnings.catch_warnings(record=True):
        warnings.simplefilter("always")
        resolved = CK.resolve_lora(sd, lora)
        before = {k: v.clone() for k, v in sd.items()}
        res = CK.merge_lora(sd, lora, 0.8, 0.6)
    assert set(resolved) == want_unet | want_clip
    assert {k for k in sd if not torch.equal(sd[k], before[k])} == set(resolved)               # merge_lora changed exactly those keys
    assert (res.unet, res.clip) == (len(want_unet), len(want_clip))
    assert resolved.unmatched == res.unmatched == ("lora_unet_not_a_layer_of_this_model",) and resolved.missing_down == res.missing_down == ()
    up, down, alpha = resolved["model.diffusion_model.input_blocks.1.0.in_layers.2.weight"]
    assert tuple(up.shape) == (64, 4, 1, 1) and tuple(down.shape) == (4, 64, 3, 3) and alpha is not None
    assert resolved["model.diffusion_model.input_blocks.2.1.transformer_blocks.0.attn2.to_k.weight"][2] is None


def test_wrongly_shaped_lora_is_refused_and_changes_nothing():
    """names that resolve but dimensions that differ (an SD2.x LoRA on this net: same block names, other attn2 / text widths): the device
    merge would index the factors by the weight's rows and columns, so they are refused on the host, where the patches are added and where
    the kernel's terms are built"""
    from lightdiffusion_amd import checkpoint as CK
    from lightdiffusion_amd import nodes
    from lightdiffusion_amd.unet import lora_factor_mismatch, lora_terms
    lora = {k: v for k, v in _lora(load_golden("lora_tiny")).items() if "not_a_layer" not in k}
    q = "lora_unet_input_blocks_1_1_transformer_blocks_0_attn1_to_q"
    k2 = "lora_unet_down_blocks_0_attentions_1_transformer_blocks_0_attn2_to_k"
    te = next(k for k in lora if k.startswith("lora_te") and k.endswith(".lora_down.weight"))
    wide = lambda t: torch.cat([t, t], dim=1)
    model, clip, unet, text = _stand_ins()
    keys = {k: torch.empty(s, device="meta") for k, s in {**model.model_key_shapes(), **clip.model_key_shapes()}.items()}
    for key, change in ((q + ".lora_down.weight", wide), (q + ".lora_down.weight", lambda t: t[:, :32]),
                        (q + ".lora_up.weight", lambda t: t[:32]), (k2 + ".lora_down.weight", wide), (te, wide)):
        bad = dict(lora)
        bad[key] = change(lora[key]).contiguous()
        with pytest.raises(ValueError, match="does not fit"):
            nodes.LoraLoader().load_lora(model, clip, bad, 0.8, 0.6)
        probe = model.clone() if not key.startswith("lora_te") else clip.clone()
        with pytest.raises(ValueError, match="does not fit"):
            probe.add_patches(CK.resolve_lora(keys, bad), 0.8)
        assert probe.patches == {} and probe.patches_uuid is None                  # nothing added, not even the keys that fit
    assert model.patches == {} and clip.patches == {} and unet.calls == [] and text.calls == []
    nodes.LoraLoader().load_lora(model, clip, lora, 0.8, 0.6)                       # (the unchanged file fits)

    # where the kernel's terms are built: the last check before raw pointers cross the ABI
    up, down = torch.randn(64, 4), torch.randn(4, 64, 3, 3)
    assert lora_factor_mismatch((64, 64, 3, 3), up, down) is None
    arr, keep = lora_terms([(up, down, 0.5)], "cpu", (64, 64, 3, 3))
    assert arr[0].rank == 4 and tuple(keep[1].shape) == (4, 576)
    for shape in ((64, 32, 3, 3), (64, 128, 3, 3), (32, 64, 3, 3), (64,)):
        with pytest.raises(ValueError, match="do not fit"):
            lora_terms([(up, down, 0.5)], "cpu", shape)
    with pytest.raises(ValueError, match="do not fit"):
        lora_terms([(torch.randn(64, 4), torch.randn(8, 576), 0.5)], "cpu", (64, 64, 3, 3))   # factors that do not chain


class _Callable(_ShapesOnly):
    def __call__(self, apply_model, params):
        self.calls.append(("forward", self.applied_patches_uuid))
        return params["input"]


def test_every_patcher_has_its_own_view_of_the_model():
    """model.apply_model swaps in the patches of the patcher the view belongs to: a clone and a second patcher built on the same SD15Model
    get views of their own, and a view kept after its patcher is gone still carries that patcher's patches"""
    import gc
    from lightdiffusion_amd import nodes
    unet = _Callable(W.unet_param_shapes(W.tiny_unet_config()))
    inner = nodes.SD15Model(unet)
    a = nodes.ModelPatcher(inner, "cpu")
    b = nodes.ModelPatcher(inner, "cpu")                                            # a second patcher on the same model object
    c = a.clone()
    assert a.model is inner and b.model is not inner and c.model is not inner
    assert a.model.diffusion_model is b.model.diffusion_model is c.model.diffusion_model is unet
    assert b.model.model_sampling is inner.model_sampling
    key = "model.diffusion_model.input_blocks.1.1.transformer_blocks.0.attn1.to_q.weight"
    patch = {key: (torch.zeros(64, 4), torch.zeros(4, 64), None)}
    assert b.add_patches(patch, 0.5) == [key] and c.add_patches(patch, 0.25) == [key]
    assert a.patches == {} and b.patches_uuid != c.patches_uuid
    x = torch.zeros(2, 4, 8, 8)
    for p in (b, a, c, a):
        p.model.apply_model(x, torch.ones(2), c_crossattn=None)
        assert unet.calls[-1] == ("forward", p.patches_uuid) and unet.applied_patches_uuid == p.patches_uuid
    view, uuid = c.model, c.patches_uuid
    del c, p
    gc.collect()
    view.apply_model(x, torch.ones(2), c_crossattn=None)
    assert unet.calls[-1] == ("forward", uuid) and unet.calls[-2][0] == "patch"


def test_lora_loader_takes_a_path_like(tmp_path):
    from lightdiffusion_amd import nodes
    lora = {k: v for k, v in _lora(load_golden("lora_tiny")).items() if "not_a_layer" not in k}
    path = pathlib.Path(tmp_path) / "lora.pt"
    torch.save(lora, path)
    model, clip, _, _ = _stand_ins()
    for name in (path, str(path)):
        m1, c1 = nodes.LoraLoader().load_lora(model, clip, name, 0.8, 0.6)
        m2, c2 = nodes.LoraLoader().load_lora(model, clip, lora, 0.8, 0.6)
        assert set(m1.patches) == set(m2.patches) != set() and set(c1.patches) == set(c2.patches) != set()
