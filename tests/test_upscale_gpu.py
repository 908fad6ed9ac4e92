"""GPU: the ESRGAN upscaler end to end: MI355XUpscaler against the reference's RRDBNet outputs, the ImageUpscaleWithModel node against the
reference's tiled_scale, the blend operator on its own, workspace growth, allocation-free forward, the launch table, and txt2img.

Allowances.  Model parity: rel-L2 of the unclamped output <= 2 x the fixture's own `emul_rel_l2` (the rel-L2 of a CPU run of the reference
that rounds weights, input and every Conv2d / LeakyReLU output to fp16: it rounds where the kernels round but sums in another order, and
the device path rounds the network input once more; a wrong tap, slope or residual scale shows as >= 1e-2).  Tiled parity: max-abs on the
clamped image <= 2 x the same emulation's largest |difference|.  The blend alone is fp32 arithmetic in the reference's order per pixel: 1e-6.
"""
import pytest
import torch

from conftest import load_golden, rel_l2
from lightdiffusion_amd import nodes as N
from lightdiffusion_amd import weights as W
from lightdiffusion_amd.upscale import MI355XUpscaler, blend_tile, tiled_upscale

pytestmark = pytest.mark.gpu

_models = {}


def model(nb, scale, seed=0):
    key = (nb, scale, seed)
    if key not in _models:
        _models[key] = N.load_synthetic_upscaler("cuda:0", nb=nb, scale=scale, seed=seed)
    return _models[key]


@pytest.mark.parametrize("name", ["esrgan_x4_nb2", "esrgan_x4_nb23", "esrgan_x2_nb1"])
def test_model_parity(name):
    g = load_golden(name)
    m = model(int(g["nb"]), int(g["scale"]), int(g["weight_seed"]))
    y = m.forward_device(g["x"]).cpu()
    assert y.shape == g["y"].shape
    err, allow = rel_l2(y, g["y"]), 2.0 * float(g["emul_rel_l2"])
    print(f"{name}: rel-L2 {err:.3e} (allowance {allow:.3e})")
    assert err <= allow, (err, allow)


def test_tiled_parity_six_tiles_and_single_tile():
    g = load_golden("esrgan_tiled")
    m = model(int(g["nb"]), int(g["scale"]), int(g["weight_seed"]))
    y6 = N.ImageUpscaleWithModel(tile=int(g["tile"]), overlap=int(g["overlap"])).upscale(m, g["x6"])[0]
    assert y6.shape == g["y6"].shape and y6.device.type == "cpu" and float(y6.min()) >= 0.0 and float(y6.max()) <= 1.0
    e6, a6 = float((y6 - g["y6"]).abs().max()), 2.0 * float(g["emul_max_abs6"])
    y1 = N.ImageUpscaleWithModel().upscale(m, g["x1"])[0]
    e1, a1 = float((y1 - g["y1"]).abs().max()), 2.0 * float(g["emul_max_abs1"])
    print(f"tiled: six tiles max-abs {e6:.3e} (allowance {a6:.3e}), single tile {e1:.3e} (allowance {a1:.3e})")
    assert e6 <= a6 and e1 <= a1
    # single tile: the mask cancels
    direct = torch.clamp(m.forward_device(g["x1"]), 0, 1).cpu()
    assert float((y1 - direct).abs().max()) <= 1e-6


def test_blend_of_the_reference_tiles_reproduces_the_reference_image():
    g = load_golden("esrgan_tiled")
    s = int(g["scale"])
    out = torch.zeros(40 * s, 56 * s, 3, device="cuda")
    div = torch.zeros(40 * s, 56 * s, device="cuda")
    for i, (y, x, h, w) in enumerate(g["rects"].tolist()):
        blend_tile(g[f"ps{i}"].cuda().contiguous(), g[f"my{i}"].cuda(), g[f"mx{i}"].cuda(), out, div, y * s, x * s)
    blend_tile(None, None, None, out, div)
    got = torch.clamp(out, 0, 1).cpu()
    assert float((got - g["y6"][0]).abs().max()) <= 1e-6


def test_workspace_growth_matches_a_fresh_model():
    small = torch.rand(1, 6, 10, 3, generator=torch.Generator().manual_seed(1))
    big = torch.rand(2, 19, 37, 3, generator=torch.Generator().manual_seed(2))
    gen = lambda name, shape: W.synth_tensor(name, shape, 3)
    a = MI355XUpscaler(W.esrgan_config(1, 2), gen, max_hw=(6, 10))
    a.forward_device(small)
    before = a.workspace_bytes
    ya = a.forward_device(big)
    assert a.workspace_bytes > before and a.workspace_bytes == a.plan_bytes(2, 19, 37)
    b = MI355XUpscaler(W.esrgan_config(1, 2), gen, max_batch=2, max_hw=(19, 37))
    assert torch.equal(ya, b.forward_device(big))


def test_forward_allocates_nothing_after_reserve():
    m = model(1, 2)
    x = torch.rand(1, 20, 24, 3).cuda()
    m.forward_device(x)
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    ws = m.workspace_bytes
    for _ in range(3):
        m.forward_device(x)
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    assert m.workspace_bytes == ws and free1 >= free0 - (1 << 20), (free0, free1)


def test_profile_names_the_kernel_and_counts_the_flops():
    nb, s, (b, h, w) = 2, 4, (1, 24, 40)
    m = model(nb, s)
    rows = m.profile(torch.rand(b, h, w, 3))
    # the trunk's convolutions: N = 32 (conv1-4) or K = 9 * 192 (conv5) at the input resolution
    dense = [r for r in rows if r[4] in ("esrgan_conv_kernel<32>", "esrgan_conv_kernel<64>")]
    assert len([r for r in dense if r[1][0] == b * h * w and (r[1][1] == 32 or r[1][2] == 9 * 192)]) == 5 * 3 * nb
    assert [r[4] for r in rows if r[0] == "upconv3"] == ["esrgan_conv_kernel<64,up>"] * 2
    assert len(rows) == m.last_launches == 15 * nb + 6
    px = b * h * w
    block = (64 + 96 + 128 + 160) * 32 + 192 * 64
    want = 2.0 * 9 * (px * (3 * 64 + 3 * nb * block + 64 * 64) + 4 * px * 64 * 64 + 16 * px * (64 * 64 + 64 * 64 + 64 * 3))
    assert m.last_flops == want, (m.last_flops, want)
    assert all(r[3] > 0 for r in rows)


def test_txt2img_with_and_without_the_upscaler():
    model_, clip, vae = N.load_synthetic("cuda:0", max_batch=1, max_hw=(8, 8), tiny=True)
    toks = [[(49406, 1.0)] + [(320, 1.0)] * 3 + [(49407, 1.0)] * 73]
    kw = dict(width=64, height=64, batch_size=1, seed=1, steps=2, cfg=3.0, sampler_name="euler_ancestral", scheduler="normal")
    base = N.txt2img(model_, clip, vae, toks, toks, **kw)
    up = N.txt2img(model_, clip, vae, toks, toks, upscale_model=model(1, 2), **kw)
    assert tuple(base.shape) == (1, 64, 64, 3) and tuple(up.shape) == (1, 128, 128, 3)
    assert float(up.min()) >= 0.0 and float(up.max()) <= 1.0
    assert torch.equal(base, N.txt2img(model_, clip, vae, toks, toks, **kw))
