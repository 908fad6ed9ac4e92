"""Time of swapping a LoRA in and out of the RESIDENT SD1.5-size UNet (record only, no threshold): a synthetic rank-16 and rank-128 LoRA over
every attention / feed-forward linear and every ResBlock convolution.

  patch + refresh      MI355XUNet.patch_weights: backup, merge kernel per weight (ld_unet_patch_param), ld_unet_refresh_derived
  unpatch + refresh    MI355XUNet.unpatch_weights: backups copied back and freed, ld_unet_refresh_derived
  reload               the only route without the device patch, in the same process: host fp32 `checkpoint.merge_lora` of those keys, then
                       ld_unet_load_param of each (upload + repack) and the refresh

Each span is bracketed by HIP events on the stream (it contains the host work queued in between) after one warm-up round; median of --reps.

    python tools/lora_patch_time.py [--out profiles/lora_patch_time.txt] [--tiny]
"""
import argparse
import os
import re
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lightdiffusion_amd import checkpoint as CK            # noqa: E402
from lightdiffusion_amd import weights as W                # noqa: E402
from lightdiffusion_amd._lib import F16, check, lib         # noqa: E402
from lightdiffusion_amd.unet import MI355XUNet              # noqa: E402

TARGETS = re.compile(r"(attn[12]\.to_(q|k|v|out\.0)|ff\.net\.0\.proj|ff\.net\.2|in_layers\.2|out_layers\.3)\.weight$")


def span(fn, reps):
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "lora_patch_time.txt"))
    ap.add_argument("--tiny", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    cfg = W.tiny_unet_config() if args.tiny else W.sd15_unet_config()
    dev = torch.device("cuda:0")
    shapes = W.unet_param_shapes(cfg)
    base = {k: W.synth_tensor(k, s, 0).half() for k, s in shapes.items()}
    unet = MI355XUNet(cfg, base, device=dev, max_batch=2, max_hw=(16, 16) if args.tiny else (64, 64))
    keys = [k for k in shapes if TARGETS.search(k)]
    nbytes = sum(2 * base[k].numel() for k in keys)
    lines = [f"LoRA swap on the resident {'tiny' if args.tiny else 'SD1.5-size'} UNet: {len(keys)} weights, {nbytes / 2**20:.0f} MiB of fp16 "
             f"(weights {unet.weight_bytes / 2**20:.0f} MiB resident); median of {args.reps} after one warm-up; ms",
             f"{'rank':>5} {'patch+refresh':>14} {'unpatch+refresh':>16} {'host merge + reload':>20} {'backup MiB':>11}"]
    stream = lambda: torch.cuda.current_stream().cuda_stream
    for rank in (16, 128):
        gen = torch.Generator().manual_seed(rank)
        lora, patches = {}, {}
        for k in keys:
            rows, cols = shapes[k][0], base[k][0].numel()
            up = (torch.randn(rows, rank, generator=gen) * 0.02).half()
            down = (torch.randn(rank, cols, generator=gen) * 0.02).half()
            name = "lora_unet_" + k[:-len(".weight")].replace(".", "_")
            lora[name + ".lora_up.weight"], lora[name + ".lora_down.weight"] = up, down
            patches[k] = [(up.to(dev), down.to(dev), 0.8)]
        unet.patch_weights(patches)                        # warm-up round
        held = unet.patch_bytes
        unet.unpatch_weights()
        t_patch, t_unpatch = [], []
        for _ in range(args.reps):
            t_patch.append(span(lambda: unet.patch_weights(patches), 1))
            t_unpatch.append(span(unet.unpatch_weights, 1))

        def reload():
            sd = {CK.UNET_PREFIX + k: (base[k].clone() if k in patches else torch.empty(shapes[k], device="meta")) for k in shapes}
            CK.merge_lora(sd, lora, 0.8)
            for k in keys:
                t = sd[CK.UNET_PREFIX + k].to(dev).contiguous()
                check(lib().ld_unet_load_param(unet._h, k.encode(), t.data_ptr(), F16, stream()), "ld_unet_load_param")
            check(lib().ld_unet_refresh_derived(unet._h, stream()), "ld_unet_refresh_derived")

        reload()                                           # warm-up
        t_reload = span(reload, args.reps)
        for k in keys:                                     # the base weights back for the next rank
            t = base[k].to(dev).contiguous()
            check(lib().ld_unet_load_param(unet._h, k.encode(), t.data_ptr(), F16, stream()), "ld_unet_load_param")
        torch.cuda.synchronize()
        lines.append(f"{rank:>5} {statistics.median(t_patch):>14.2f} {statistics.median(t_unpatch):>16.2f} {t_reload:>20.1f} {held / 2**20:>11.0f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
