"""CPU: the host side of the ESRGAN upscaler: key normalisation and config detection, the tile plan and feather ramps against the
reference's (tests/golden/esrgan_tiled.npz), and tests/esrgan_ref.py against the reference's model outputs."""
import pytest
import torch

import esrgan_ref as ER
from conftest import load_golden, rel_l2
from lightdiffusion_amd import checkpoint as CK
from lightdiffusion_amd import weights as W
from lightdiffusion_amd.upscale import feather_ramp, tile_plan


def _sd(nb=2, scale=4, seed=0):
    return W.synth_state_dict(W.esrgan_param_shapes(W.esrgan_config(nb, scale)), seed)


@pytest.mark.parametrize("scale,nb", [(4, 2), (2, 1), (4, 23)])
def test_three_spellings_normalise_to_the_same_parameters(scale, nb):
    old = _sd(nb, scale)
    for style in ("old", "trunk", "body"):
        sd = ER.respell(old, style, nb, scale)
        for wrapped in (sd, {"params_ema": sd}, {"module." + k: v for k, v in sd.items()}):
            got = CK.normalize_esrgan_keys(wrapped)
            assert set(got) == set(old), (style, set(got) ^ set(old))
            assert all(got[k] is old[k] for k in old)
            assert CK.detect_esrgan_config(wrapped) == W.esrgan_config(nb, scale)


def test_rejections_name_their_reason():
    sd = ER.respell(_sd(1, 2), "body", 1, 2)
    with pytest.raises(ValueError, match="conv1x1"):
        CK.detect_esrgan_config({**sd, "body.0.rdb1.conv1x1.weight": torch.zeros(32, 64, 1, 1)})
    with pytest.raises(ValueError, match="in_nc = 12"):
        CK.detect_esrgan_config({**sd, "conv_first.weight": torch.zeros(64, 12, 3, 3)})
    with pytest.raises(ValueError, match="out_nc = 1"):
        CK.detect_esrgan_config({**sd, "conv_last.weight": torch.zeros(1, 64, 3, 3)})
    with pytest.raises(ValueError, match="nf = 32"):
        CK.detect_esrgan_config({**sd, "conv_first.weight": torch.zeros(32, 3, 3, 3)})
    with pytest.raises(ValueError, match="gc = 16"):
        CK.detect_esrgan_config({**sd, "body.0.rdb1.conv1.weight": torch.zeros(16, 64, 3, 3)})
    with pytest.raises(ValueError, match="not an RRDBNet"):
        CK.detect_esrgan_config({"conv.weight": torch.zeros(1)})


def test_tile_plan_and_ramps_equal_the_reference():
    g = load_golden("esrgan_tiled")
    tile, overlap, scale = int(g["tile"]), int(g["overlap"]), int(g["scale"])
    plan = tile_plan(40, 56, tile, overlap)
    assert plan == [tuple(int(v) for v in r) for r in g["rects"]]
    assert [(h, w) for _, _, h, w in plan] == [(32, 32), (32, 32), (32, 8), (16, 32), (16, 32), (16, 8)]
    feather = round(overlap * scale)
    for i, (_, _, h, w) in enumerate(plan):
        assert torch.equal(feather_ramp(h * scale, feather), g[f"my{i}"])
        assert torch.equal(feather_ramp(w * scale, feather), g[f"mx{i}"])
    assert [(h, w) for _, _, h, w in tile_plan(512, 512, 512, 32)] == [(512, 512), (512, 32), (32, 512), (32, 32)]
    assert tile_plan(24, 40, 512, 32) == [(0, 0, 24, 40)]


@pytest.mark.parametrize("name", ["esrgan_x4_nb2", "esrgan_x4_nb23", "esrgan_x2_nb1"])
def test_restatement_reproduces_the_reference(name):
    """fp32 on the CPU: the same arithmetic in another order (fp32 reassociation only)."""
    g = load_golden(name)
    nb, scale = int(g["nb"]), int(g["scale"])
    y = ER.rrdbnet(_sd(nb, scale, int(g["weight_seed"])), g["x"], nb, scale)
    assert y.shape == g["y"].shape
    assert rel_l2(y, g["y"]) < 1e-5
    assert 1e-4 < float(g["emul_rel_l2"]) < 5e-3


@pytest.mark.parametrize("name", ["esrgan_x2_nb1", "esrgan_x4_nb2"])
def test_fp16_emulation_mode_reproduces_the_fixtures_emulation(name):
    """rrdbnet(emulate_fp16=True) rounds where the fixtures' emulation rounded (weights, input, every Conv2d / LeakyReLU output): its distance from
    the reference's fp32 output is the fixture's own `emul_rel_l2` up to fp32 summation noise — the allowance the chain tests derive from this
    mode for the scales that have no fixture (tests/test_esrgan_chain_gpu.py) is measured the way the fixtures' was."""
    g = load_golden(name)
    nb, scale = int(g["nb"]), int(g["scale"])
    sd = _sd(nb, scale, int(g["weight_seed"]))
    mine, stored = rel_l2(ER.rrdbnet(sd, g["x"], nb, scale, emulate_fp16=True), g["y"]), float(g["emul_rel_l2"])
    print(f"{name}: emulation rel-L2 {mine:.6e}, the fixture's emul_rel_l2 {stored:.6e}")
    assert abs(mine - stored) <= 1e-2 * stored, (mine, stored)
    assert rel_l2(ER.rrdbnet(sd, g["x"], nb, scale), g["y"]) < 1e-5          # the default mode is untouched


@pytest.mark.parametrize("nb,scale,shape", [(1, 1, (2, 6, 10)), (1, 1, (1, 17, 9)), (1, 8, (1, 3, 5))])
def test_fp16_emulation_distance_at_the_scales_without_a_fixture(nb, scale, shape):
    """The same measurement at scale 1 and scale 8, on the chain tests' shapes: of the order the fixtures store (rand images in [0, 1])."""
    sd = _sd(nb, scale)
    x = torch.rand(*shape, 3, generator=torch.Generator().manual_seed(7))
    y = ER.rrdbnet(sd, x, nb, scale)
    assert tuple(y.shape) == (shape[0], shape[1] * scale, shape[2] * scale, 3)
    e = rel_l2(ER.rrdbnet(sd, x, nb, scale, emulate_fp16=True), y)
    print(f"x{scale} nb{nb} {shape}: emulation rel-L2 {e:.3e}")
    assert 1e-4 < e < 5e-3
