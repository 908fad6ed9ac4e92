"""GPU: the Detailer on the device.
  (a) detailer.do_detail with the closed-form stand-in stages over lightdiffusion_amd.ops against the reference's two recorded runs
      (tests/golden/detailer_flow.npz), compared as tests/test_detailer_cpu.py compares the NumPy ops;
  (b) nodes.DetailerForEach on the tiny synthetic model: every segment's encoder tile, alpha and pasted canvas against the NumPy restatement
      (detailer_ref, usdu_ref) applied to the device's own canvas and decoded image; the 5-tuple; the seed index; the host generator;
  (c) the node's rejections are do_detail's.

THE CANVAS BOUND.  The device's alpha and the reference's differ by at most B = detailer_ref.blur_bound(feather) (two blurs of the same mask
within the derived bound of the exact one).  The paste canvas' = (1 - a) canvas + a t, with canvas and t in [0, 1], moves by at most B |t -
canvas| <= B under that, and each side evaluates it in fp32 with every operation rounded: 1 - a and the two products lie in [0, 1] and are each
off by at most half an ulp there, 2^-25; the sum by at most 2^-24; that is 2.5 * 2^-24 a side and 5 * 2^-24 for the two sides, whose roundings
need not agree once the alphas differ.  Canvases and final images: B + 5 * 2^-24.  Tiles are bitwise: the fixture asserts that no pixel of the
overlap sits within the blur bound of a byte boundary."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detailer_ref as R                                       # noqa: E402
import detailer_standins as S                                  # noqa: E402
import usdu_ref as U                                           # noqa: E402
from test_detailer_cpu import GOLDEN, bits, flow_segs          # noqa: E402
from lightdiffusion_amd import detailer as D                   # noqa: E402
from lightdiffusion_amd import nodes as N                      # noqa: E402
from lightdiffusion_amd import ops                             # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOKS = [[(49406, 1.0)] + [(320, 1.0)] * 3 + [(49407, 1.0)] * 73]


def canvas_bound(feather):
    return R.blur_bound(feather) + 5 * 2.0 ** -24               # module docstring


@pytest.fixture(scope="module")
def flow_golden():
    return np.load(os.path.join(GOLDEN, "detailer_flow.npz"))


def f64(t):
    return (t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).astype(np.float64)


# ------------------------------------------------------------------ (a) the stand-in stages on the device ops
@pytest.mark.parametrize("tag", ["plain", "disc"])
def test_do_detail_with_standin_stages_on_the_device_ops(flow_golden, tag):
    flow = flow_golden
    image, segs = flow_segs()
    if tag == "disc":
        segs = D.segs_bitwise_and_mask(segs, S.flow_disc())
    p = S.flow_params()
    blur, bound = R.blur_bound(p["feather"]), canvas_bound(p["feather"])
    seen, worst = [], {"alpha": 0.0, "canvas": 0.0}

    def observe(o):
        j = len(seen)
        seen.append(o.index)
        assert o.alpha.is_cuda and o.tile.is_cuda and o.canvas.is_cuda, "the segment's images stay on the device"
        assert o.seed == int(flow[tag + "_seed"][j]) == p["seed"] + o.index
        assert list(o.crop) == list(flow[tag + "_crop"][j]) and list(o.work_size) == list(flow[tag + "_size"][j]) == list(o.size)
        assert np.array_equal(o.tile.cpu().numpy(), flow[f"{tag}_tile_{j}"]), f"segment {o.index}: encoder tile"
        x1, y1, x2, y2 = o.crop
        worst["alpha"] = max(worst["alpha"], float(np.abs(f64(o.alpha) - flow[f"{tag}_alpha_{j}"]).max()))
        worst["canvas"] = max(worst["canvas"], float(np.abs(f64(o.canvas[y1:y2, x1:x2]) - flow[f"{tag}_after_{j}"]).max()))

    before = image.clone()
    final, cropped, enhanced, enhanced_alpha, cnet, (shape, new_segs) = D.do_detail(
        image, segs, None, None, None, p["guide_size"], p["guide_size_for_bbox"], p["max_size"], p["seed"], p["steps"], p["cfg"], p["sampler_name"],
        p["scheduler"], [], [], p["denoise"], p["feather"], p["noise_mask"], p["force_inpaint"], "", cycle=p["cycle"], inpaint_model=False,
        noise_mask_feather=p["noise_mask_feather"], stages=S.standin_stages(ops, DEV, observe))
    print(f"{tag}: mask error {worst['alpha']:.3e} (bound {blur:.3e}), canvas error {worst['canvas']:.3e} (bound {bound:.3e})")
    assert worst["alpha"] <= blur and worst["canvas"] <= bound
    assert seen == S.FLOW_DETAILED and torch.equal(image, before), "the input image is not written"
    assert final.device.type == "cpu" and final.dtype == torch.float32 and tuple(final.shape) == tuple(image.shape)
    want = image[0].numpy().copy()
    outside = np.ones(S.FLOW_SHAPE, bool)
    for j, (x1, y1, x2, y2) in enumerate(flow[tag + "_crop"]):
        want[y1:y2, x1:x2] = flow[f"{tag}_after_{j}"]
        outside[y1:y2, x1:x2] = False
    assert float(np.abs(f64(final[0]) - want).max()) <= bound
    assert np.array_equal(bits(final[0].numpy()[outside]), bits(image[0].numpy()[outside])), "pixels outside every crop are the input's"
    assert cnet == [] and tuple(shape) == S.FLOW_SHAPE
    assert len(cropped) == len(enhanced) == len(enhanced_alpha) == len(new_segs) == len(S.FLOW_DETAILED)
    for j in range(len(cropped)):                                                  # the lists: sorted by shape, largest first, as recorded
        assert tuple(cropped[j].shape) == tuple(flow[f"{tag}_cropped_{j}"].shape) == tuple(enhanced[j].shape)
        assert float(np.abs(f64(cropped[j]) - flow[f"{tag}_cropped_{j}"]).max()) <= bound
        assert np.array_equal(bits(enhanced[j].numpy()), bits(R.to_f32(flow[f"{tag}_enhanced_{j}"])))
        assert tuple(enhanced_alpha[j].shape) == tuple(enhanced[j].shape[:3]) + (4,) and torch.equal(enhanced_alpha[j][..., :3], enhanced[j])
        assert float(np.abs(f64(enhanced_alpha[j][..., 3]) - flow[f"{tag}_enhanced_alpha_{j}"]).max()) <= blur
    assert [list(s.crop_region) for s in new_segs] == [list(c) for c in flow[tag + "_new_seg_crop"]]


# ------------------------------------------------------------------ (b) the node on the tiny model
@pytest.fixture(scope="module")
def tiny():
    model, clip, vae = N.load_synthetic(DEV, max_batch=1, max_hw=(8, 8), tiny=True)
    cond, pooled = clip.encode_from_tokens(TOKS, return_pooled=True)
    return model, clip, vae, [[cond, {"pooled_output": pooled}]]


def doit(tiny, image, segs, feather=5, wildcard="", **kw):
    model, clip, vae, cond = tiny
    p = S.flow_params()
    return N.DetailerForEach().doit(image, segs, model, clip, vae, p["guide_size"], p["guide_size_for_bbox"], p["max_size"], p["seed"], 4, p["cfg"],
                                    p["sampler_name"], p["scheduler"], cond, cond, p["denoise"], feather, p["noise_mask"], p["force_inpaint"], wildcard,
                                    **kw)


def test_node_on_the_tiny_model(tiny, monkeypatch):
    image, (shape, items) = flow_segs()
    segs = (shape, items[:3])                          # 0 and 2 do not overlap; 1 has an all-zero mask: skipped, but it takes seed + 1
    p = S.flow_params()
    feather, blur, bound = p["feather"], R.blur_bound(p["feather"]), canvas_bound(p["feather"])
    rec = SimpleNamespace(prev=image[0].numpy().copy(), decoded=[], seen=[], encode_rng=[], sample_rng=[], built=0)
    build = D.model_stages

    def model_stages(*a, **kw):
        st = build(*a, **kw)
        assert st.ops is ops and st.device == torch.device(DEV)
        rec.built += 1
        encode, sample, decode = st.encode, st.sample, st.decode

        def enc(px):
            rec.encode_rng.append(torch.get_rng_state())
            return encode(px)

        def smp(latent, seed):
            out = sample(latent, seed)
            rec.sample_rng.append(torch.get_rng_state())
            return out

        def dec(latent):
            out = decode(latent)
            rec.decoded.append(out.detach().clone())
            return out
        st.encode, st.sample, st.decode, st.observe = enc, smp, dec, observe
        return st

    def observe(o):
        j = len(rec.seen)
        rec.seen.append((o.index, o.seed))
        seg = segs[1][o.index]
        x1, y1, x2, y2 = o.crop
        assert list(o.crop) == list(seg.crop_region) and o.work_size == (64, 64)
        # the encoder tile: the NumPy chain on the canvas as it was before this segment, bitwise
        tile = U.resample(R.crop_u8(rec.prev, x1, y1, x2, y2), 64, 64, "lanczos")
        assert np.array_equal(o.tile.cpu().numpy(), tile), f"segment {o.index}: encoder tile"
        alpha = R.gaussian_blur(seg.cropped_mask, feather).astype(np.float32)
        err_a = float(np.abs(f64(o.alpha) - f64(alpha)).max())
        # the paste: the reference's, of the device's own decoded image resized back, with the reference's alpha
        assert len(rec.decoded) == j + 1 and tuple(rec.decoded[j].shape) == (1, 64, 64, 3)
        back = ops.u8_resample(ops.u8_from_f32(rec.decoded[j].to(DEV, torch.float32))[0], (x2 - x1, y2 - y1), "lanczos").cpu().numpy()
        want = R.paste(rec.prev.copy(), back, alpha, x1, y1)
        got = o.canvas.cpu().numpy()
        err_c = float(np.abs(f64(got) - f64(want)).max())
        print(f"segment {o.index}: alpha error {err_a:.3e} (bound {blur:.3e}), canvas error {err_c:.3e} (bound {bound:.3e})")
        assert err_a <= blur and err_c <= bound
        outside = np.ones(S.FLOW_SHAPE, bool)
        outside[y1:y2, x1:x2] = False
        assert np.array_equal(bits(got[outside]), bits(rec.prev[outside])), "the paste stays inside the crop"
        assert not np.array_equal(bits(got[~outside]), bits(rec.prev[~outside])), "the segment was redrawn"
        rec.prev = got.copy()

    monkeypatch.setattr(D, "model_stages", model_stages)
    before = image.clone()
    torch.manual_seed(3)
    out = doit(tiny, image, segs)
    after_rng = torch.get_rng_state()
    assert rec.built == 1 and rec.seen == [(0, p["seed"]), (2, p["seed"] + 2)], "the skipped segment still advances the seed index"
    assert isinstance(out, tuple) and len(out) == 5 and torch.equal(image, before)
    enhanced, cropped, cropped_enhanced, cropped_enhanced_alpha, cnet = out
    assert enhanced.device.type == "cpu" and enhanced.dtype == torch.float32 and tuple(enhanced.shape) == (1,) + S.FLOW_SHAPE + (3,)
    assert np.array_equal(bits(enhanced[0].numpy()), bits(rec.prev)), "the returned image is the last canvas"
    assert [tuple(t.shape) for t in cropped] == [(1, 64, 64, 3), (1, 32, 32, 3)] == [tuple(t.shape) for t in cropped_enhanced]      # largest first
    assert [tuple(t.shape) for t in cropped_enhanced_alpha] == [(1, 64, 64, 4), (1, 32, 32, 4)]
    for seg, crop in zip((items[2], items[0]), cropped):
        x1, y1, x2, y2 = seg.crop_region
        assert torch.equal(crop[0], image[0, y1:y2, x1:x2]), "cropped: the crop before its redraw (these two do not overlap)"
    for e, ea in zip(cropped_enhanced, cropped_enhanced_alpha):
        assert torch.equal(ea[..., :3], e) and float(ea[..., 3].min()) >= 0.0 and float(ea[..., 3].max()) <= 1.0 + blur
        assert np.array_equal(bits(e.numpy()), bits(R.to_f32(S.as_u8(e)))), "enhanced crops hold k / 255"
    assert len(cnet) == 1 and tuple(cnet[0].shape) == (1, 64, 64, 3) and cnet[0].dtype == torch.float32 and not cnet[0].any()
    # the host generator, as test_host_generator_is_consumed_as_the_reference_consumes_it has it: GaussianBlur's sigma draw once per segment
    # before the empty-mask test and once per detailed segment — so two draws lie before segment 0's encode, and three (segment 1's one,
    # segment 2's two) between the end of segment 0's sampling (which re-seeds: prepare_noise) and segment 2's encode
    assert len(rec.encode_rng) == len(rec.sample_rng) == 2

    def state_after(start, draws):
        if start is None:
            torch.manual_seed(3)
        else:
            torch.set_rng_state(start)
        for _ in range(draws):
            torch.empty(1).uniform_(10.0, 10.0)
        return torch.get_rng_state()
    assert torch.equal(rec.encode_rng[0], state_after(None, 2))
    assert torch.equal(rec.encode_rng[1], state_after(rec.sample_rng[0], 3))
    assert not torch.equal(rec.encode_rng[1], state_after(rec.sample_rng[0], 2))
    assert torch.equal(after_rng, rec.sample_rng[1]), "nothing is drawn after the last segment"


# ------------------------------------------------------------------ (c) the rejections
def test_node_rejections_are_do_details(tiny):
    image, segs = flow_segs()
    with pytest.raises(ValueError, match="batch of 2"):
        doit(tiny, torch.cat([image, image]), segs)
    with pytest.raises(ValueError, match="segs were made for"):
        doit(tiny, image[:, :100], segs)
    with pytest.raises(ValueError, match="feather=32"):
        doit(tiny, image, segs, feather=32)                                          # the smallest crop is 32 x 32
    with pytest.raises(ValueError, match="feather=-1"):
        doit(tiny, image, segs, feather=-1)
    with pytest.raises(ValueError, match="wildcard_opt"):
        doit(tiny, image, segs, wildcard="blue eyes")
    for name, value in [("detailer_hook", object()), ("inpaint_model", True), ("scheduler_func_opt", lambda *a: None)]:
        with pytest.raises(ValueError, match=name):
            doit(tiny, image, segs, **{name: value})
    with pytest.raises(ValueError, match="cycle=0"):
        doit(tiny, image, segs, cycle=0)
    with pytest.raises(ValueError, match="control_net_wrapper"):
        doit(tiny, image, (segs[0], [segs[1][0]._replace(control_net_wrapper=object())]))
    with pytest.raises(ValueError, match="crop region"):
        doit(tiny, image, (segs[0], [segs[1][0]._replace(crop_region=[240, 0, 272, 32])]))
    with pytest.raises(ValueError, match="image"):
        doit(tiny, image[..., :2], segs)
    out = doit(tiny, image, (segs[0], []), wildcard=None)                            # no segments: the image back, a copy; None is "" (wildcard_opt)
    assert torch.equal(out[0], image) and out[0] is not image and out[1] == out[2] == out[3] == [] and len(out[4]) == 1
    with pytest.raises(ValueError, match="stages"):                                  # do_detail itself still needs its stages
        D.do_detail(image, segs, None, None, None, 64, False, 128, 7, 4, 3.0, "euler_ancestral", "normal", [], [], 0.5, 5, True, True)
