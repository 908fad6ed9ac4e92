"""ControlNet on the device against the operator chains at SD1.5's full width: the one-image step and a 512 x 768 request of four images, per
launch and per bit; every stage element-wise against fp64.

The harness is tests/test_controlnet_chain_gpu.py's (its `Side`, `launches_held`, `graph_laps`, `stages`), the sizes those of
tests/test_unet_chain_full_gpu.py: the routes the product runs.  What is new against that module are the 13 zero convolutions (a single-source
1x1 at K = 320 / 640 / 1280 on 2 nb x (64 x 64 .. 8 x 8) rows), the hint encoder on a 512 x 512 / 768 x 512 image and the control add over 13
segments; ZERO_ROUTES names the kernel every level's zero convolution runs on, read off the tables the cases print (no split over K
but at the 8 x 8 level of two images; no halo tile and no row-resident kernel: those take 3x3 convolutions only).

B1, B2 (with the other case in between, and under the replayed graph), B3 as in tests/test_controlnet_chain_gpu.py.
    Layers held under an exception: none.
B3 of sd15_pair4_96x64 evaluates the stages that are separable per image on images IMAGES of the 8 (chain_harness.tap_images); the other
    images of those taps are not looked at by B3 — B2 still holds their bits.  The hint encoder (one image), the time embedding, conv_in, the
    control adds, the pair split and conv_out are evaluated whole.  B3's wall time goes into the record beside the figures.
The taps of one case are kept at a time (Side's one_case_taps).
"""
import json
import time

import pytest
import torch

import chain_harness as H
import test_controlnet_chain_gpu as T

pytestmark = pytest.mark.gpu

# name -> (config, nb, (h, w), tokens, mode, hint batch, strength)
CASES = {
    "sd15_pair1_64x64": ("sd15", 1, (64, 64), 77, "pair", 1, 1.0),         # the one-image step
    "sd15_pair4_96x64": ("sd15", 4, (96, 64), 77, "pair", 1, 1.0),         # 192 tiles, H != W at every level
}
IMAGES = {"sd15_pair1_64x64": H.EVERY_IMAGE, "sd15_pair4_96x64": (0, -1)}

side = H.side_fixture(lambda tag: T.Side(tag, cases=CASES, one_case_taps=True))

# the kernel every level's zero convolution runs on, [(count, kernel)] in the order the branch runs them (input blocks 0 .. 11, middle_block_out)
_DEEP, _G64, _G128, _2WG = "gemm3_kernel<64,160,conv,deep>", "gemm3_kernel<64,160,conv>", "gemm3_kernel<128,160,conv>", "gemm4_kernel<64,64,conv,2wg>"
ZERO_ROUTES = {
    # 2 images.  320 @ 64 x 64: 128 panels x 2 = 256 tiles, deep's one round; 320 / 640 @ 32 x 32: 64 / 128 tiles; 640 @ 16 x 16: 32 tiles, deep;
    # 1280 @ 16 x 16: 512 rows = 160 tiles of 64 x 64, skinny_conv1; 1280 @ 8 x 8: 16 tiles, deep, two slices over K
    "sd15_pair1_64x64": [(3, _DEEP), (3, _G64), (1, _DEEP), (2, _2WG), (4, _DEEP + "+splitk_reduce_kernel")],
    # 8 images.  320 @ 96 x 64: 384 panels of 128 x 2 = 768 tiles; 320 @ 48 x 32: 192 panels x 2 = 384 tiles, deep's one round; 640 @ 48 x 32 and
    # 24 x 16: 768 / 192 tiles; 1280 @ 24 x 16: 48 panels x 8 = 384 tiles, deep; 1280 @ 12 x 8: 768 rows = 240 tiles of 64 x 64, skinny_conv1
    "sd15_pair4_96x64": [(3, _G128), (1, _DEEP), (3, _G64), (2, _DEEP), (4, _2WG)],
}
REACHES = {name: T._ALWAYS + ("dup_halves_kernel",) for name in CASES}


@pytest.mark.parametrize("name", list(CASES))
def test_same_launches(side, name):
    T.launches_held(name, side("sd15"), REACHES[name], ZERO_ROUTES[name])


@pytest.mark.parametrize("name", list(CASES))
def test_same_bits(side, name):
    s = side("sd15")
    want = s.chain_out(name)
    H.same_bits(name, want, s.executor_run, [o for o in CASES if o != name])
    T.graph_laps(name, s, want)


@pytest.mark.parametrize("name", list(CASES))
def test_every_stage_elementwise(side, name):
    s = side("sd15")
    s.chain_run(name)
    n_all = 2 * CASES[name][1]
    images = IMAGES[name]
    assert images != H.EVERY_IMAGE or n_all <= 4, f"{name}: a case of {n_all} images names its subset"
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rec, fails, count = T.stages(name, s, images=images)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    print(f"PARITY {name}: " + json.dumps(rec) + f" images {H.image_indices(images, n_all)} B3 {seconds:.1f} s")
    H.record(T.RECORD, name, dict(rec, images_checked=H.image_indices(images, n_all), b3_seconds=round(seconds, 1)))
    assert not fails, f"{len(fails)} of {count} stages outside their bound:\n" + "\n".join(fails[:12])
