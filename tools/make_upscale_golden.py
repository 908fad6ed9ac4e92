"""Writes the ESRGAN fixtures of tests/golden/ from the reference's own RRDBNet and tiled_scale.

The reference is read where it lies (LD_REFERENCE, as oracle/extract_ref.py does): the file is parsed and a whitelist of its top-level
definitions is executed in a namespace of torch names; none of its text is copied.  ImageUpscaleWithModel.upscale itself asks for
torch.cuda.current_device(), so tiled_scale + clamp are called here with the node's arguments.  Weights are weights.synth_tensor values
(no ESRGAN checkpoint exists offline) and are not stored: every fixture holds inputs, fp32 reference outputs and the seeds.

    python tools/make_upscale_golden.py
"""
import ast
import functools
import math
import os
import re
import sys
from collections import OrderedDict
from typing import Literal, Union

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from lightdiffusion_amd import weights as W   # noqa: E402
import esrgan_ref as ER                        # noqa: E402
from oracle.extract_ref import REF_PATH        # noqa: E402

NAMES = {"act", "get_valid_padding", "ShortcutBlock", "sequential", "ConvMode", "conv_block", "RRDB", "ResidualDenseBlock_5C", "upconv_block",
         "RRDBNet", "get_tiled_scale_steps", "tiled_scale"}
GOLDEN = os.path.join(ROOT, "tests", "golden")


def load_reference():
    ns = {"torch": torch, "nn": nn, "re": re, "math": math, "functools": functools, "OrderedDict": OrderedDict, "Literal": Literal, "Union": Union,
          "__name__": "ld_reference_upscale"}
    tree = ast.parse(open(REF_PATH).read(), REF_PATH)
    found = set()
    for node in tree.body:
        name = getattr(node, "name", None)
        if name is None and isinstance(node, ast.Assign) and isinstance(node.targets[0], ast.Name):
            name = node.targets[0].id
        if name in NAMES:
            exec(compile(ast.Module([node], []), REF_PATH, "exec"), ns)
            found.add(name)
    if NAMES - found:
        raise RuntimeError(f"reference symbols not found: {sorted(NAMES - found)}")
    return ns


def half_round(t):
    return t.half().float()


def emulated(ns, sd):
    """The reference model with weights, and every Conv2d / LeakyReLU output, rounded to fp16: where the device path rounds."""
    m = ns["RRDBNet"]({k: half_round(v) for k, v in sd.items()}).eval()
    for mod in m.modules():
        if isinstance(mod, (nn.Conv2d, nn.LeakyReLU)):
            mod.register_forward_hook(lambda _m, _i, o: half_round(o))
    return lambda x: m(half_round(x))


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def ramp(n, feather):
    """One axis of the feather mask of an n-pixel tile, n >= feather: (k + 1) / feather over the first and, mirrored, the last `feather`
    pixels, the two multiplied where they overlap; each factor rounded to fp32 before the product, as a float tensor takes a Python scalar."""
    assert n >= feather
    k = np.arange(n)
    side = lambda d: np.where(d < feather, (1.0 / feather) * (d + 1), 1.0).astype(np.float32)
    return side(k) * side(n - 1 - k)


def image(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def main():
    ns = load_reference()
    torch.set_grad_enabled(False)
    nchw = lambda t: t.permute(0, 3, 1, 2).contiguous()
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()

    def models(nb, scale, seed, style):
        sd = ER.respell(W.synth_state_dict(W.esrgan_param_shapes(W.esrgan_config(nb, scale)), seed), style, nb, scale)
        ref = ns["RRDBNet"](OrderedDict(sd)).eval()
        assert ref.scale == scale and ref.num_blocks == nb, (ref.scale, ref.num_blocks)
        return ref, emulated(ns, OrderedDict(sd))

    for fname, nb, scale, shape, style in (("esrgan_x4_nb2", 2, 4, (1, 24, 40, 3), "body"), ("esrgan_x4_nb23", 23, 4, (1, 24, 40, 3), "body"),
                                           ("esrgan_x2_nb1", 1, 2, (2, 17, 23, 3), "trunk")):
        ref, emu = models(nb, scale, 0, style)
        x = image(shape, 1)
        y = nhwc(ref(nchw(x)))
        e = rel_l2(nhwc(emu(nchw(x))), y)
        print(f"{fname}: out {tuple(y.shape)}, emul_rel_l2 {e:.3e}")
        np.savez_compressed(os.path.join(GOLDEN, fname + ".npz"), x=x.numpy(), y=y.numpy(), nb=nb, scale=scale, weight_seed=0, image_seed=1,
                            emul_rel_l2=np.float64(e))

    # tiled_scale: x2, nb 2; six tiles (tile 32 / overlap 8 on 40 x 56) and the node defaults on 24 x 40 (one tile)
    nb, scale = 2, 2
    ref, emu = models(nb, scale, 0, "body")
    out = dict(nb=nb, scale=scale, weight_seed=0, image_seed=2, tile=32, overlap=8)
    x6 = image((1, 40, 56, 3), 2)
    tiles = []

    def recording(a):
        ps = ref(a)
        tiles.append(nhwc(ps)[0].numpy())
        return ps

    node = lambda fn, x, tile, overlap: torch.clamp(ns["tiled_scale"](nchw(x), fn, tile_x=tile, tile_y=tile, overlap=overlap, upscale_amount=scale)
                                                    .movedim(-3, -1), min=0, max=1.0)
    y6 = node(recording, x6, 32, 8)
    e6 = float((node(emu, x6, 32, 8) - y6).abs().max())
    step = 32 - 8
    rects = [(y, x, min(32, 40 - y), min(32, 56 - x)) for y in range(0, 40, step) for x in range(0, 56, step)]
    assert len(rects) == len(tiles) == ns["get_tiled_scale_steps"](56, 40, 32, 32, 8)
    feather = round(8 * scale)
    acc, div = torch.zeros_like(y6[0]), torch.zeros(y6.shape[1], y6.shape[2], 1)
    for i, (r, ps) in enumerate(zip(rects, tiles)):
        assert ps.shape[:2] == (r[2] * scale, r[3] * scale)
        out[f"my{i}"], out[f"mx{i}"], out[f"ps{i}"] = ramp(ps.shape[0], feather), ramp(ps.shape[1], feather), ps
        m = torch.from_numpy(np.outer(out[f"my{i}"], out[f"mx{i}"]))[..., None]
        win = (slice(r[0] * scale, (r[0] + r[2]) * scale), slice(r[1] * scale, (r[1] + r[3]) * scale))
        acc[win] += torch.from_numpy(ps) * m
        div[win] += m
    # the separated ramps and the rectangles, blended here, are the reference's mask: they reproduce its image from its own tiles
    assert float((torch.clamp(acc / div, 0, 1) - y6[0]).abs().max()) <= 1e-6
    out.update(x6=x6.numpy(), y6=y6.numpy(), rects=np.array(rects, dtype=np.int64), emul_max_abs6=np.float64(e6))
    x1 = image((1, 24, 40, 3), 3)
    y1 = node(ref, x1, 512, 32)
    e1 = float((node(emu, x1, 512, 32) - y1).abs().max())
    out.update(x1=x1.numpy(), y1=y1.numpy(), emul_max_abs1=np.float64(e1))
    print(f"esrgan_tiled: six tiles {[tuple(r[2:]) for r in rects]}, emul max-abs {e6:.3e} (six tiles), {e1:.3e} (single tile)")
    np.savez_compressed(os.path.join(GOLDEN, "esrgan_tiled.npz"), **out)


if __name__ == "__main__":
    main()
