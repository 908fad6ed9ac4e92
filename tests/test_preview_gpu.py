"""GPU: the TAESD latent preview end to end: MI355XTAESD against the reference's TAESD.decode, the uint8 image, graph replay against eager,
workspace growth, allocation-free decode, the launch count, and txt2img with a LatentPreviewer.

Allowances (those of tests/test_upscale_gpu.py, by the same reasoning).  Model parity: rel-L2 of the decode <= 2 x the fixture's own
`emul_rel_l2` and max-abs <= 2 x `emul_max_abs`: the distances from the reference's fp32 run of a CPU run of the reference that rounds
weights, input and every Conv2d output to fp16: it rounds where the kernels round but sums in another order; a missing ReLU, skip or tap
shows as >= 1e-2.  The image is the formula on the device's own fp32 decode, bit for bit, and so differs from the fixture's image by at
most ceil(255 * emul_max_abs) counts ((d + 1) / 2 halves the decode's allowance, 255 scales it, truncation adds under one count).
"""
import math

import pytest
import torch

import taesd_ref as TR
from conftest import load_golden, rel_l2
from lightdiffusion_amd import nodes as N
from lightdiffusion_amd import weights as W
from lightdiffusion_amd.preview import LatentPreviewer, MI355XTAESD

pytestmark = pytest.mark.gpu

LAUNCHES = 35          # first + 3 x (3 Blocks x 3 + upsampling convolution) + 3 (the last Block) + last
_models = {}


def model(seed=0):
    if seed not in _models:
        _models[seed] = N.load_synthetic_taesd("cuda:0", seed=seed, max_hw=(17, 33), max_batch=2)
    return _models[seed]


@pytest.mark.parametrize("name", ["taesd_9x13", "taesd_b2_17x33"])
def test_model_parity_and_image(name):
    g = load_golden(name)
    m = model(int(g["weight_seed"]))
    d = m.decode(g["x"])
    assert d.shape == g["y"].shape and d.dtype == torch.float32 and d.is_cuda
    assert m.last_launches == LAUNCHES
    err, allow = rel_l2(d.cpu(), g["y"]), 2.0 * float(g["emul_rel_l2"])
    mx, mallow = float((d.cpu() - g["y"]).abs().max()), 2.0 * float(g["emul_max_abs"])
    img = m.image(g["x"])
    assert img.shape == g["image"].shape and img.dtype == torch.uint8 and img.is_cuda
    counts = int((img.cpu().int() - g["image"].int()).abs().max())
    callow = math.ceil(255.0 * float(g["emul_max_abs"]))
    print(f"{name}: rel-L2 {err:.3e} (allowance {allow:.3e}), max-abs {mx:.3e} (allowance {mallow:.3e}), image {counts} counts (allowance {callow})")
    assert err <= allow, (err, allow)
    assert mx <= mallow, (mx, mallow)
    assert torch.equal(img, TR.to_image(d)), "the image is not the formula on the device's own decode"
    assert counts <= callow, (counts, callow)


def test_graph_replay_equals_eager_on_a_second_latent():
    m = model()
    gen = torch.Generator().manual_seed(5)
    lat = [torch.randn(2, 4, 9, 13, generator=gen).cuda() * s for s in (1.0, 4.0)]
    got = {True: [], False: []}
    for use_graph in (True, False):
        pv = LatentPreviewer(m, lambda i, im, k=use_graph: got[k].append((i, im)), rows=slice(0, 2), use_graph=use_graph)
        for i, x in enumerate(lat):
            pv({"x": x, "i": i, "sigma": 1.0, "denoised": None})
        assert (pv._graph is not None) == use_graph
    assert [i for i, _ in got[True]] == [0, 1]
    for (_, a), (_, b), x in zip(got[True], got[False], lat):
        assert a.dtype == torch.uint8 and tuple(a.shape) == (2, 72, 104, 3) and not a.is_cuda
        assert torch.equal(a, b)
        assert torch.equal(a, m.image(x).cpu())
    assert not torch.equal(got[True][0][1], got[True][1][1])


def test_workspace_growth_matches_a_fresh_model():
    gen = lambda name, shape: W.synth_tensor("taesd_decoder." + name, shape, 3)
    small = torch.randn(1, 4, 3, 5, generator=torch.Generator().manual_seed(1))
    big = torch.randn(2, 4, 9, 13, generator=torch.Generator().manual_seed(2))
    a = MI355XTAESD(gen, max_hw=(3, 5))
    a.decode(small)
    before = a.workspace_bytes
    ya = a.decode(big)
    assert a.workspace_bytes > before and a.workspace_bytes == a.plan_bytes(2, 9, 13)
    b = MI355XTAESD(gen, max_batch=2, max_hw=(9, 13))
    assert torch.equal(ya, b.decode(big))


def test_decode_allocates_nothing_after_reserve():
    m = model()
    x = torch.randn(1, 9, 13, 4).cuda()
    out = torch.empty(1, 72, 104, 3, device="cuda")
    img = torch.empty(1, 72, 104, 3, dtype=torch.uint8, device="cuda")
    m.decode_into(x, out, img)
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    ws = m.workspace_bytes
    for _ in range(3):
        m.decode_into(x, out, img)
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    assert m.workspace_bytes == ws and free1 >= free0 - (1 << 20), (free0, free1)


def test_profile_names_the_kernels_and_counts_the_flops():
    m = model()
    b, h, w = 1, 9, 13
    rows = m.profile(torch.randn(b, 4, h, w))
    assert len(rows) == m.last_launches == LAUNCHES
    names = [r[4] for r in rows]
    assert names[0] == "taesd_first_kernel" and names[-1] == "taesd_last_kernel"
    assert names.count("taesd_conv_kernel") == 30 and names.count("taesd_conv_kernel<up>") == 3
    assert [i for i, k in enumerate(names) if k == "taesd_conv_kernel<up>"] == [10, 20, 30]
    px = b * h * w
    want = 2.0 * 9 * (px * 4 * 64 + 64 * 64 * (9 * px + 10 * 4 * px + 10 * 16 * px + 4 * 64 * px) + 64 * px * 64 * 3)
    assert m.last_flops == want, (m.last_flops, want)
    assert all(r[3] > 0 for r in rows)


@pytest.mark.parametrize("sampler,scheduler", [("euler_ancestral", "normal"), ("dpmpp_2m_sde", "karras")])
def test_txt2img_with_a_preview_keeps_the_trajectory(sampler, scheduler):
    if "sd" not in _models:
        _models["sd"] = N.load_synthetic("cuda:0", max_batch=1, max_hw=(8, 8), tiny=True)
    model_, clip, vae = _models["sd"]
    toks = [[(49406, 1.0)] + [(320, 1.0)] * 3 + [(49407, 1.0)] * 73]
    lat = N.EmptyLatentImage().generate(64, 64, 1)[0]
    enc = lambda t: clip.encode_from_tokens(t, return_pooled=True)
    (pc, pp), (nc, npool) = enc(toks), enc(toks)
    pos, neg = [[pc, {"pooled_output": pp}]], [[nc, {"pooled_output": npool}]]
    args = (model_, 1, 4, 3.0, sampler, scheduler, pos, neg, lat)
    got = []
    pv = LatentPreviewer(model(), lambda i, im: got.append((i, im)))
    with_preview = N.KSampler2().sample(*args, preview=pv)[0]["samples"]
    assert [i for i, _ in got] == [0, 1, 2, 3]
    assert all(im.dtype == torch.uint8 and tuple(im.shape) == (1, 64, 64, 3) and not im.is_cuda for _, im in got)
    assert torch.equal(with_preview, N.KSampler2().sample(*args)[0]["samples"]), "the preview disturbed the trajectory"
    kw = dict(width=64, height=64, batch_size=1, seed=1, steps=4, cfg=3.0, sampler_name=sampler, scheduler=scheduler)
    got.clear()
    img = N.txt2img(model_, clip, vae, toks, toks, preview=pv, **kw)
    assert len(got) == 4 and torch.equal(img, N.txt2img(model_, clip, vae, toks, toks, **kw))
