"""Model and tiled parity of the ESRGAN upscaler against the reference's goldens, with the allowances of tests/test_upscale_gpu.py
-> profiles/upscale_parity.json.    python tools/upscale_parity.py [out.json]"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_golden, rel_l2          # noqa: E402
from lightdiffusion_amd import nodes as N         # noqa: E402


def main():
    out = {"model_rel_l2": {}, "tiled_max_abs": {}}
    for name in ("esrgan_x4_nb2", "esrgan_x4_nb23", "esrgan_x2_nb1"):
        g = load_golden(name)
        m = N.load_synthetic_upscaler("cuda:0", nb=int(g["nb"]), scale=int(g["scale"]), seed=int(g["weight_seed"]))
        out["model_rel_l2"][name] = {"measured": rel_l2(m.forward_device(g["x"]).cpu(), g["y"]), "emulation": float(g["emul_rel_l2"]),
                                     "allowance": 2.0 * float(g["emul_rel_l2"])}
    g = load_golden("esrgan_tiled")
    m = N.load_synthetic_upscaler("cuda:0", nb=int(g["nb"]), scale=int(g["scale"]), seed=int(g["weight_seed"]))
    y6 = N.ImageUpscaleWithModel(tile=int(g["tile"]), overlap=int(g["overlap"])).upscale(m, g["x6"])[0]
    y1 = N.ImageUpscaleWithModel().upscale(m, g["x1"])[0]
    for key, y, ref, emu in (("six_tiles", y6, g["y6"], g["emul_max_abs6"]), ("single_tile", y1, g["y1"], g["emul_max_abs1"])):
        out["tiled_max_abs"][key] = {"measured": float((y - ref).abs().max()), "emulation": float(emu), "allowance": 2.0 * float(emu)}
    text = json.dumps(out, indent=1)
    print(text)
    with open(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "upscale_parity.json"), "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
