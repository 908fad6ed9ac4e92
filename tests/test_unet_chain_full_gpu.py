"""The UNet executor against the operator chain (tests/unet_chain.py) at SD1.5's full width: the benchmark step, the one-image step, the hires
step and the two non-square requests (512 x 768 and 768 x 512), per launch and per bit; every stage element-wise against fp64.

The harness is that of tests/test_unet_chain_gpu.py (its `Side`, its `_stage` references, tests/chain_harness.py); what differs is the size.
From about 192 tiles or row panels on the planner leaves the routes the 16 x 16 cases of that module run and takes the ones the product runs
on: the halo-tile convolution (+groupnorm, plain, with split-K and the finishing pass that writes GroupNorm partials), the K = 320 row-panel
GEMMs (plain, ln, geglu+ln), the 256 x 320 tiles (geglu, conv), the folded up-convolution with its reduce, the 8-wave attention, and at two
images the row-resident convolution from 64 pixels down.  The launch tables the cases print are the authority; REACHES pins them.
B3 of the hires case on two images takes 2.4 s against 1.8 s of the 96 x 64 case: it is kept for all five cases.

B1  same launches, against profile_pair's launch table entry by entry; REACHES: the routes a case is in the table for, NEVER: the ones it is
    in the table for NOT taking (landscape: neither the halo tile nor the row-resident kernel has a tile for a 96-pixel row).
B2  same bits, with every other case of this module run in between on the same handle (A, B, A) and under the hipGraph the wrapper hook
    replays (two laps).  No tolerance.
    Layers held under an exception instead (a seam call reproducing the launch, held to B3's element bound): none.
B3  every tap against the fp64 reference of that one stage, the bounds of tests/errbound.py, no new bound.  A case of more than 4 images
    evaluates the references of the stages that are separable per image (GroupNorm's statistics, every convolution, attention, the rows of
    a linear: the taps that carry their image count) on a FIXED subset of images, IMAGES below: the first and the last image of the tensor —
    one from each half of the pair once it is split, all rows of both — one image at a time (chain_harness.tap_images).  Up to 4 images: all of
    them, one at a time.  The other images of those taps are not looked at by B3 (B2 still holds their bits to the chain's).  The time
    embedding, conv_in with the pair's second copy, the pair split (`dup`) and conv_out are evaluated whole, on all images.
    With LD_WRITE_PARITY=1 the worst error / bound and signed bias per stage kind, the images checked and B3's wall time go to
    profiles/unet_chain_parity.json under the case name (a record).
Completeness: every contraction instantiation the three profiled SD1.5 forwards of tests/test_routes_gpu.py dispatch (8 and 1 at 64 x 64,
    4 at 128 x 128, CFG pairs) appears in the chain's launch lists of this module; a route a retune introduces has to come with a case.

The taps of one case are kept at a time (Side's one_case_taps): the chain is run again where another test asks for them, and has to return
the bits it returned before.
"""
import json
import time

import pytest
import torch

import chain_harness as H
import test_unet_chain_gpu as U
from test_routes_gpu import _contraction

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# name -> (config, nb, (h, w), tokens, mode); every case a CFG pair of nb latents: 2 nb images
CASES = {
    "sd15_pair4_96x64": ("sd15", 4, (96, 64), 77, "pair"),       # 8 x 6144 rows: exactly 192 halo tiles and 192 row panels; H != W at every level
    "sd15_pair8_64x64": ("sd15", 8, (64, 64), 77, "pair"),       # the benchmark step
    "sd15_pair1_64x64": ("sd15", 1, (64, 64), 77, "pair"),       # the one-image step: the row-resident convolution from 64 pixels down
    "sd15_pair1_64x96": ("sd15", 1, (64, 96), 77, "pair"),       # landscape: the general tiles at full width
    "sd15_pair4_128x128": ("sd15", 4, (128, 128), 77, "pair"),   # the hires step: 128-pixel bands
}
# the images B3 evaluates of a tap that is separable per image (negative: from the end)
IMAGES = {
    "sd15_pair4_96x64": (0, -1),
    "sd15_pair8_64x64": (0, -1),
    "sd15_pair1_64x64": H.EVERY_IMAGE,
    "sd15_pair1_64x96": H.EVERY_IMAGE,
    "sd15_pair4_128x128": (0, -1),
}


def inputs(name):
    tag, nb, (h, w), tokens, mode = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    x = (torch.randn(nb, 4, h, w, generator=g) * 3.0).to(DEV)
    sigma = torch.tensor([U.SIGMAS[i % len(U.SIGMAS)] for i in range(nb)], dtype=torch.float32, device=DEV)
    ctx = torch.randn(2 * nb, tokens, U.config(tag)["context_dim"], generator=g).to(DEV)
    return x, sigma, ctx


side = H.side_fixture(lambda tag: U.Side(tag, cases=CASES, inputs_of=inputs, one_case_taps=True))
_LAUNCHES = {}


def chain_launches(s, name):
    """[(layer, kernel)] of the chain's run of the case (kept per case: the taps are not)."""
    if name not in _LAUNCHES:
        _, taps = s.chain_run(name)
        _LAUNCHES[name] = [(t["name"], k) for t in taps for k in t["launches"].split(";") if k]
    return _LAUNCHES[name]


# ------------------------------------------------------------------ B1

# kernel names (prefixes) and layer-name suffixes, read off the launch tables the cases print ("+skip": a ResBlock whose 1x1 skip is a second K
# segment of out_layers' convolution; ".skip_connection": the skip as a launch of its own)
_ALWAYS = tuple(k for k in U._ALWAYS if k != "+skip") + ("dup_halves_kernel",)
_FILLED = ("+skip", "gemm7_kernel<256,K320,plain>", "gemm7_kernel<256,K320,plain,ln>", "gemm7_kernel<256,K320,geglu,ln>", "gemm5_kernel<256,320,geglu>",
           "flash_attn2_kernel<3,rowV,plain,8>", "flash_attn2_kernel<3,masked,8>", "conv6_kernel<W32,halo>+splitk_reduce_gn_kernel",
           "upconv_kernel<256,320>+upconv_reduce_kernel", "gn_stats_kernel+gn_finalize_kernel")
_GENERAL = ("gemm4_kernel<64,64,conv,2wg>", "gemm3_kernel<64,160,conv,deep>+splitk_reduce_gn_kernel", "flash_attn2_kernel<3,rowV,plain,4>")
REACHES = {
    "sd15_pair4_96x64": _ALWAYS + _FILLED + ("conv6_kernel<W64,halo+groupnorm>", "gemm3_kernel<64,160,conv,deep>"),
    "sd15_pair8_64x64": _ALWAYS + _FILLED + ("conv6_kernel<W64,halo+groupnorm>", "conv6_kernel<W16,halo>+splitk_reduce_gn_kernel"),
    "sd15_pair1_64x64": _ALWAYS + _GENERAL + ("conv8_kernel<W64>", "conv8_kernel<W32>", "conv8_kernel<W32,up>", "conv8_kernel<W16>", "conv8_kernel<W16,up>",
                                              "conv8_kernel<W8>", ".skip_connection"),
    "sd15_pair1_64x96": _ALWAYS + _GENERAL + ("+skip", "gemm3_kernel<64,160,conv,deep>", "gemm3_kernel<128,160,conv>+splitk_reduce_kernel"),
    "sd15_pair4_128x128": _ALWAYS + _FILLED + ("conv6_kernel<W128,halo+groupnorm>", "conv6_kernel<W64,halo>", "gemm5_kernel<256,320,conv>",
                                               "conv6_kernel<W16,halo>+splitk_reduce_gn_kernel"),
}
# portrait: the row-resident kernel takes Ho == Wo only; landscape: a 96-, 48- or 24-pixel row is no tile width of the halo tile either
NEVER = {
    "sd15_pair4_96x64": ("conv8_kernel", "conv6_kernel<W16"),
    "sd15_pair1_64x96": ("conv6_kernel", "conv8_kernel"),
}


@pytest.mark.parametrize("name", list(CASES))
def test_same_launches(side, name):
    s = side(CASES[name][0])
    _, taps = s.chain_run(name)
    mine = H.same_launches(name, taps, s.executor_table(name))
    _LAUNCHES[name] = mine
    names = {k for _, k in mine}
    layers = [t["name"] for t in taps]
    print(f"LAUNCHES {name}: {sorted(names)}")
    for want in REACHES[name]:
        assert any(k.startswith(want) for k in names) or any(l.endswith(want) for l in layers), f"{name} no longer reaches {want}: {sorted(names)}"
    for bad in NEVER.get(name, ()):
        assert not any(bad in k for k in names), f"{name} was to run without {bad}: {sorted(names)}"


def test_chain_cases_cover_the_profiled_forwards(side):
    """Every contraction instantiation of the three forwards test_unet_forward_routes_are_pinned profiles is launched by a case above."""
    s = side("sd15")
    mine = set()
    for name in CASES:
        for _, k in chain_launches(s, name):
            mine.add(k)
            mine.update(k.split("+"))
    for batch, hw in ((8, 64), (1, 64), (4, 128)):
        s.unet.set_context(torch.randn(2 * batch, 77, 768))
        s.unet.profile_pair(torch.randn(batch, 4, hw, hw, device=DEV), torch.full((batch,), 3.0, device=DEV))
        seen = {k for k in s.unet.profile_kernels() if _contraction(k)}
        assert seen, "no contraction kernels profiled"
        missing = sorted(seen - mine)
        assert not missing, f"the pair of {batch} at {hw} x {hw} dispatches what no chain case of this module launches: {missing}"


# ------------------------------------------------------------------ B2

@pytest.mark.parametrize("name", list(CASES))
def test_same_bits(side, name):
    tag, nb, (h, w), tokens, mode = CASES[name]
    s = side(tag)
    want = s.chain_out(name)
    H.same_bits(name, want, s.executor_run, [o for o in CASES if o != name])
    # the captured graph the model_function_wrapper hook replays, first contact and a replay (as tests/test_unet_chain_gpu.py)
    x, sigma, ctx = inputs(name)
    x, sigma = torch.cat([x, x]).contiguous(), torch.cat([sigma, sigma]).contiguous()
    params = {"input": x, "timestep": sigma, "c": {"c_crossattn": ctx, "transformer_options": {}}, "cond_or_uncond": [1, 0]}
    s.unet._hook.clear()
    for lap in (0, 1):
        got = s.unet(None, params)
        assert s.unet._hook[(x.shape[0], h, w)].pair.graph is not None
        H.bits_held(got, want, f"{name} under the replayed graph, lap {lap}")
    s.unet._hook.clear()


# ------------------------------------------------------------------ B3

@pytest.mark.parametrize("name", list(CASES))
def test_every_stage_elementwise(side, name):
    s = side(CASES[name][0])
    _, taps = s.chain_run(name)
    n_all = 2 * CASES[name][1]
    images = IMAGES[name]
    assert images != H.EVERY_IMAGE or n_all <= 4, f"{name}: a case of {n_all} images names its subset"
    kinds = {t["kind"] for t in taps}
    assert kinds == {"timestep", "linear", "conv_in", "conv_out", "groupnorm", "conv", "upconv", "gn_conv", "linear_ln", "attention", "dup"}, kinds
    whole = {t["kind"] for t in taps if "n" not in t}
    assert whole == {"timestep", "linear", "conv_in", "conv_out", "dup"}, f"stages evaluated on all images: {whole}"
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rec, fails = H.every_stage(name, taps, lambda tap, what: U._stage(tap, s.chain, what), images=images)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    print(f"PARITY {name}: " + json.dumps(rec) + f" images {H.image_indices(images, n_all)} B3 {seconds:.1f} s")
    H.record("unet_chain_parity.json", name, dict(rec, images_checked=H.image_indices(images, n_all), b3_seconds=round(seconds, 1)))
    H.stages_held(fails, taps)
