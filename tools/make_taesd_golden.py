"""Writes the TAESD fixtures of tests/golden/ from the reference's own TAESD.

The reference is read where it lies (oracle.extract_ref.REF_PATH): the file is parsed and a whitelist of its top-level definitions is
executed in a namespace of torch names; none of its text is copied.  The namespace's `load_torch_file` returns the synthetic state dict,
so `TAESD()` loads our weights through its own constructor.  Weights are weights.synth_tensor("taesd_decoder." + key) values (no TAESD
file exists offline) and are not stored: every fixture holds the latent, the reference's fp32 decode, its uint8 image, the key / shape
list, the seeds, and the distance of an fp16-rounding emulation of the reference from its fp32 run.

    python tools/make_taesd_golden.py
"""
import ast
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from lightdiffusion_amd import weights as W   # noqa: E402
import taesd_ref as TR                         # noqa: E402
from oracle.extract_ref import REF_PATH        # noqa: E402

NAMES = {"cast_bias_weight", "CastWeightBiasOp", "disable_weight_init", "conv", "Clamp", "Block", "Encoder2", "Decoder2", "TAESD"}
GOLDEN = os.path.join(ROOT, "tests", "golden")
WEIGHT_SEED = 0


def load_reference(state_dict):
    ns = {"torch": torch, "nn": nn, "load_torch_file": lambda *a, **k: state_dict, "__name__": "ld_reference_taesd"}
    tree = ast.parse(open(REF_PATH).read(), REF_PATH)
    found = set()
    for node in tree.body:
        name = getattr(node, "name", None)
        if name not in NAMES:
            continue
        if name == "conv" and [a.arg for a in node.args.args] != ["n_in", "n_out"]:     # TAESD's own helper, not another module's
            continue
        exec(compile(ast.Module([node], []), REF_PATH, "exec"), ns)
        found.add(name)
    if NAMES - found:
        raise RuntimeError(f"reference symbols not found: {sorted(NAMES - found)}")
    return ns


def half_round(t):
    return t.half().float()


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def main():
    torch.set_grad_enabled(False)
    shapes = W.taesd_decoder_param_shapes()
    sd = {k: W.synth_tensor("taesd_decoder." + k, s, WEIGHT_SEED) for k, s in shapes.items()}
    ref = load_reference(sd)["TAESD"]().eval()
    emu = load_reference({k: half_round(v) for k, v in sd.items()})["TAESD"]().eval()
    for mod in emu.taesd_decoder.modules():
        if isinstance(mod, nn.Conv2d):
            mod.register_forward_hook(lambda _m, _i, o: half_round(o))
    got = {k: tuple(v.shape) for k, v in ref.taesd_decoder.state_dict().items()}
    assert got == shapes and list(got) == list(shapes), "weights.taesd_decoder_param_shapes() is not Decoder2's state dict"
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()
    keys = np.array(list(shapes))
    shp = np.array([list(s) + [0] * (4 - len(s)) for s in shapes.values()], dtype=np.int64)
    for fname, shape, scale, seed in (("taesd_9x13", (1, 4, 9, 13), 1.0, 1), ("taesd_b2_17x33", (2, 4, 17, 33), 8.0, 1)):
        x = scale * torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)
        y = nhwc(ref.decode(x))
        ye = nhwc(emu.decode(half_round(x)))
        img = TR.to_image(y)
        e, m = rel_l2(ye, y), float((ye - y).abs().max())
        unsat = float(((img > 0) & (img < 255)).float().mean())
        print(f"{fname}: out {tuple(y.shape)}, std {float(y.std()):.3f}, |x| max {float(x.abs().max()):.1f}, unsaturated bytes {unsat:.2f}, "
              f"emul rel-L2 {e:.3e} max-abs {m:.3e}")
        np.savez_compressed(os.path.join(GOLDEN, fname + ".npz"), x=x.numpy(), y=y.numpy(), image=img.numpy(), keys=keys, shapes=shp,
                            weight_seed=WEIGHT_SEED, latent_seed=seed, emul_rel_l2=np.float64(e), emul_max_abs=np.float64(m))


if __name__ == "__main__":
    main()
