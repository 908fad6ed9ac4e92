"""Parity of the two LoRA routes against the reference's patched model on the `lora_tiny` fixture (record only; the bounds are those of
tests/test_configs_gpu.py::test_lora_merged_unet_and_clip_match_reference, which tests/test_lora_patch_gpu.py asserts for the device route):

  device_patch       plain load, then nodes.LoraLoader on the loaded stack: the merge kernel on the resident fp16 weights
  load_time_merge    CheckpointLoaderSimple.load_checkpoint(lora=...): host fp32 merge of the state dict before the upload

Both at strengths 0.8 / 0.6 on the fp32 synthetic base; UNet: rel-L2 of one denoising step against `denoised`, CLIP: rel-L2 of the hidden
state at layer -2 against `clip_inter_m2`.

    python tools/lora_patch_parity.py [--out profiles/lora_patch_parity.json]
"""
import argparse
import json
import os
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))             # the fixture's set-up lives with the tests that share it
from conftest import load_golden, rel_l2                    # noqa: E402
from test_host_cpu import _lora_from_golden, _synthetic_checkpoint   # noqa: E402
from lightdiffusion_amd import nodes                        # noqa: E402
from lightdiffusion_amd import weights as W                 # noqa: E402

DEV = "cuda:0"


def measure(model, clip, g):
    unet = model.patch_model().diffusion_model
    unet.set_context(g["ctx"])
    den = unet.forward(g["x"].to(DEV), g["sigma"].to(DEV)).cpu()
    inter = clip.patch_model()(g["tokens"], intermediate_output=-2)[1].cpu()
    return {"unet_rel_l2": rel_l2(den, g["denoised"]), "clip_rel_l2": rel_l2(inter, g["clip_inter_m2"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "lora_patch_parity.json"))
    args = ap.parse_args()
    g = load_golden("lora_tiny")
    lora = _lora_from_golden(g)
    sd, ucfg, _, ccfg = _synthetic_checkpoint()
    sd.update({"model.diffusion_model." + k: v for k, v in W.synth_state_dict(W.unet_param_shapes(ucfg)).items()})   # fp32 base weights
    loader = nodes.CheckpointLoaderSimple(DEV, max_batch=1, max_hw=(16, 16), clip_heads=ccfg["num_attention_heads"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                     # (the fixture carries one module that matches no layer, on purpose)
        model, clip, _ = loader.load_checkpoint(dict(sd))
        device = measure(*nodes.LoraLoader().load_lora(model, clip, lora, 0.8, 0.6), g)
        del model, clip
        merged = measure(*loader.load_checkpoint(dict(sd), lora=lora, lora_strength=0.8, lora_strength_clip=0.6)[:2], g)
    rec = {"fixture": "tests/golden/lora_tiny.npz, strengths 0.8 / 0.6, fp32 base", "written_by": "tools/lora_patch_parity.py",
           "bounds": {"unet_rel_l2": 5e-3, "clip_rel_l2": 5e-3}, "device_patch": device, "load_time_merge": merged}
    text = json.dumps(rec, indent=1) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
