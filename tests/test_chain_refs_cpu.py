"""CPU controls of the ESRGAN and TAESD chains (tests/esrgan_chain.py, tests/taesd_chain.py; tests/test_esrgan_chain_gpu.py,
tests/test_taesd_chain_gpu.py): the host-only module walks against counts derived from the config and against the key lists of
weights.esrgan_param_shapes / taesd_decoder_param_shapes, and the stage references the chains' taps are held with (dense_conv_ref,
taesd_conv_ref) against an fp32 emulation of the stage with the kernels' single fp16 rounding — which must stay inside the bound on every
element — and against that emulation with one defect planted, which must not.  The defects are what an executor could get wrong between
the kernel tests and the output tests: a residual scale, a residual taken from the wrong buffer, a stale channel, the epilogue's order.
Shapes are those of the chains' case tables.
"""
import pytest
import torch
import torch.nn.functional as F

import chain_harness as H
import esrgan_chain as EC
import taesd_chain as TC
from lightdiffusion_amd import weights as W
from test_esrgan_conv_gpu import dense_conv_ref
from test_taesd_conv_gpu import taesd_conv_ref


# ------------------------------------------------------------------ module walks

@pytest.mark.parametrize("nb,scale", [(1, 1), (1, 2), (2, 4), (1, 8), (23, 4)])
def test_esrgan_modules_walk(nb, scale):
    cfg = W.esrgan_config(nb, scale)
    mods = EC.modules(cfg)
    n_up = {1: 0, 2: 1, 4: 2, 8: 3}[scale]
    assert len(mods) == 15 * nb + 4 + n_up
    kinds = [m[0] for m in mods]
    assert kinds[0] == "first" and kinds[-2:] == ["hr", "last"] and kinds.count("up") == n_up and kinds.count("trunk") == 1
    assert kinds.count("dense") == 12 * nb and kinds.count("conv5") == 3 * nb
    assert kinds[1:1 + 15 * nb] == (["dense"] * 4 + ["conv5"]) * (3 * nb) and kinds[1 + 15 * nb] == "trunk"
    shapes = W.esrgan_param_shapes(cfg)
    assert [k for _, name, _, _ in mods for k in (name + ".weight", name + ".bias")] == list(shapes)
    for _, name, cin, cout in mods:
        assert shapes[name + ".weight"] == (cout, cin, 3, 3) and shapes[name + ".bias"] == (cout,)
    assert [(cin, cout) for k, _, cin, cout in mods[1:6]] == [(64, 32), (96, 32), (128, 32), (160, 32), (192, 64)]


def test_taesd_modules_walk():
    mods = TC.modules()
    assert len(mods) == 35 == 1 + 3 * (3 * 3 + 1) + 3 + 1
    kinds = [m[0] for m in mods]
    assert kinds[0] == "first" and kinds[-1] == "last" and [i for i, k in enumerate(kinds) if k == "up"] == [10, 20, 30] and kinds.count("conv") == 30
    shapes = W.taesd_decoder_param_shapes()
    keys = [k for kind, name, _, _ in mods for k in ((name + ".weight",) if kind == "up" else (name + ".weight", name + ".bias"))]
    assert keys == list(shapes) and len(keys) == 67
    for _, name, cin, cout in mods:
        assert shapes[name + ".weight"] == (cout, cin, 3, 3)


# ------------------------------------------------------------------ the stage references against planted defects

def _rand(shape, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).half()


def _conv32(x_nhwc, w, b, up=False):
    """fp32 convolution of fp16 operands, NHWC in, [n h w][cout] out."""
    x = x_nhwc.float().permute(0, 3, 1, 2)
    if up:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    y = F.conv2d(x, w.float(), None if b is None else b.float(), padding=1)
    return y.permute(0, 2, 3, 1).reshape(-1, w.shape[0])


def _check(y32, ref, bound, what, h, w):
    return H.held(y32.half(), ref, bound, what, image_rows=h * w, width=w)


def _caught(y32, ref, bound, what, h, w):
    with pytest.raises(AssertionError, match="element bound"):
        _check(y32, ref, bound, what, h, w)


@pytest.mark.parametrize("n,h,w", [(1, 5, 7), (2, 9, 11), (1, 17, 33)])
def test_esrgan_stage_references_reject_planted_defects(n, h, w):
    """An RRDB's third block at the network's scales: activations of order 1, the synthetic checkpoint's weights."""
    cfg = W.esrgan_config(1, 2)
    shapes = W.esrgan_param_shapes(cfg)
    wt = lambda name: W.synth_tensor(name + ".weight", shapes[name + ".weight"]).half()
    bs = lambda name: W.synth_tensor(name + ".bias", shapes[name + ".bias"]).half()
    dense = _rand((n, h, w, 192), 10 * h + w)                        # x | x1 .. x4 of this block
    stale = _rand((n, h, w, 192), 10 * h + w + 1)                    # what the buffer held before: the block before last's x1 .. x4
    rrdb_in = _rand((n, h, w, 64), 10 * h + w + 2)
    c5 = "model.1.sub.0.RDB3.conv5.0"
    x, r1 = dense, dense[..., :64]
    flat = lambda t: t.float().reshape(-1, t.shape[-1])
    ref, bound = dense_conv_ref(x, wt(c5), bs(c5), 0.0, [(0.2, r1), (0.2, rrdb_in)])
    v = _conv32(x, wt(c5), bs(c5))
    good = 0.2 * (0.2 * v + flat(r1)) + flat(rrdb_in)
    _check(good, ref, bound, "conv5 R1 + R2", h, w)
    _caught(0.2 * (v + flat(r1)) + flat(rrdb_in), ref, bound, "conv5 without the 0.2 on R1", h, w)
    _caught(0.2 * v + flat(r1), ref, bound, "R2 dropped", h, w)
    _caught(0.2 * (0.2 * v + flat(r1)) + flat(r1), ref, bound, "R2 from the block's input instead of rrdb_in", h, w)
    # the first two blocks of an RRDB: R1 alone
    ref1, bound1 = dense_conv_ref(x, wt(c5), bs(c5), 0.0, [(0.2, r1)])
    _check(0.2 * v + flat(r1), ref1, bound1, "conv5 R1", h, w)
    _caught(v + flat(r1), ref1, bound1, "conv5 R1 without the 0.2", h, w)
    # convolution 3 appends behind 128 channels; the defect reads ONE channel the block has not written yet (x2's last, still the stale value)
    c3 = "model.1.sub.0.RDB3.conv3.0"
    xin = dense[..., :128]
    ref3, bound3 = dense_conv_ref(xin, wt(c3), bs(c3), 0.2)
    _check(F.leaky_relu(_conv32(xin, wt(c3), bs(c3)), 0.2), ref3, bound3, "conv3", h, w)
    bad = xin.clone()
    bad[..., 127] = stale[..., 127]
    _caught(F.leaky_relu(_conv32(bad, wt(c3), bs(c3)), 0.2), ref3, bound3, "a stale x2 channel read as input", h, w)
    _caught(_conv32(xin, wt(c3), bs(c3)), ref3, bound3, "no LeakyReLU", h, w)
    # the trunk convolution + the ShortcutBlock's add, and an up-convolution
    tr = "model.1.sub.1"
    trunk_in = _rand((n, h, w, 64), 10 * h + w + 3)
    reft, boundt = dense_conv_ref(dense[..., :64], wt(tr), bs(tr), 0.0, [(1.0, trunk_in)])
    _check(_conv32(dense[..., :64], wt(tr), bs(tr)) + flat(trunk_in), reft, boundt, "trunk", h, w)
    _caught(_conv32(stale[..., :64], wt(tr), bs(tr)) + flat(trunk_in), reft, boundt, "the trunk convolution on the other dense buffer", h, w)
    up = "model.3"
    refu, boundu = dense_conv_ref(dense[..., :64], wt(up), bs(up), 0.2, up=True)
    _check(F.leaky_relu(_conv32(dense[..., :64], wt(up), bs(up), up=True), 0.2), refu, boundu, "upconv", 2 * h, 2 * w)


@pytest.mark.parametrize("n,h,w", [(1, 3, 5), (3, 2, 2), (2, 9, 13), (1, 17, 33)])
def test_taesd_stage_references_reject_planted_defects(n, h, w):
    """A Block's third convolution and an up-convolution: non-negative inputs (they follow a ReLU), the synthetic checkpoint's weights."""
    shapes = W.taesd_decoder_param_shapes()
    wt = lambda name: W.synth_tensor(TC.PREFIX + name + ".weight", shapes[name + ".weight"]).half()
    b3 = W.synth_tensor(TC.PREFIX + "3.conv.4.bias", (64,)).half()
    x = _rand((n, h, w, 64), 20 * h + w).clamp_min(0)                 # the Block's input
    t1 = _rand((n, h, w, 64), 20 * h + w + 1).clamp_min(0)
    t2 = _rand((n, h, w, 64), 20 * h + w + 2).clamp_min(0)
    flat = lambda t: t.float().reshape(-1, 64)
    ref, bound = taesd_conv_ref(t2, wt("3.conv.4"), b3, x, True, False)
    v = _conv32(t2, wt("3.conv.4"), b3)
    _check(F.relu(v + flat(x)), ref, bound, "Block conv 3", h, w)
    _caught(F.relu(v + flat(t1)), ref, bound, "residual from t1 instead of x", h, w)
    _caught(F.relu(v) + flat(x), ref, bound, "ReLU before the residual add", h, w)
    _caught(F.relu(_conv32(t1, wt("3.conv.4"), b3) + flat(x)), ref, bound, "the third convolution reads t1", h, w)
    refu, boundu = taesd_conv_ref(x, wt("7"), None, None, False, True)
    vu = _conv32(x, wt("7"), None, up=True)
    _check(vu, refu, boundu, "up-convolution", 2 * h, 2 * w)
    _caught(vu + b3.float(), refu, boundu, "up-convolution with a bias", 2 * h, 2 * w)
    _caught(F.relu(vu), refu, boundu, "up-convolution with a ReLU", 2 * h, 2 * w)
