"""GPU parity of the whole hot path through the C ABI: UNet step (apply_model), the wrapper-hook contract, VAE decode.
Goldens come from the reference's own classes (fp32, CPU).  The HIP path stores activations/weights in fp16 with fp32
accumulation, like the reference's GPU dtype policy (LD.py:6418-6423); SURVEY §8c measured the reference's own
fp16-vs-fp32 gap at rel-L2 1.8e-3 per UNet call, so the bound here is rel-L2 <= 5e-3 per call."""
import pytest
import torch

from conftest import load_golden, rel_l2
from lightdiffusion_amd import weights as W
from oracle import sd15_ref as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
UNET_TOL = 5e-3


@pytest.fixture(scope="module")
def tiny_unet():
    from lightdiffusion_amd.unet import synthetic_unet
    return synthetic_unet(W.tiny_unet_config(), max_batch=4, max_hw=(16, 16))


@pytest.mark.parametrize("name", ["unet_tiny_16x16", "unet_tiny_8x12"])
def test_tiny_unet_golden(tiny_unet, name):
    g = load_golden(name)
    tiny_unet.set_context(g["ctx"])
    x, s = g["x"].to(DEV), g["sigma"].to(DEV)
    eps = tiny_unet.forward(x, s, eps_only=True).cpu()
    den = tiny_unet.forward(x, s).cpu()
    assert rel_l2(eps, g["eps"]) < UNET_TOL
    assert rel_l2(den, g["denoised"]) < UNET_TOL
    assert torch.isfinite(den).all()


def test_tiny_unet_batch4_matches_batch2(tiny_unet):
    """samples are independent: a batch of 4 = two batches of 2 (what the 8-GPU sharding relies on).  Not bitwise:
    tile / split-K choices follow the GEMM M dimension, so the fp32 summation order differs between batch sizes."""
    g = load_golden("unet_tiny_16x16")
    x = torch.cat([g["x"], g["x"].flip(0)]).to(DEV)
    s = torch.cat([g["sigma"], g["sigma"].flip(0)]).to(DEV)
    ctx = torch.cat([g["ctx"], g["ctx"].flip(0)])
    tiny_unet.set_context(ctx)
    d4 = tiny_unet.forward(x, s).cpu()
    tiny_unet.set_context(g["ctx"])
    d2 = tiny_unet.forward(g["x"].to(DEV), g["sigma"].to(DEV)).cpu()
    assert rel_l2(d4[:2], d2) < 3e-3 and rel_l2(d4[2:], d2.flip(0)) < 3e-3
    d2b = tiny_unet.forward(g["x"].to(DEV), g["sigma"].to(DEV)).cpu()
    assert torch.equal(d2, d2b), "same inputs, same shape: the step must be bitwise reproducible"


def test_forward_pair_equals_forward_on_duplicated_inputs(tiny_unet):
    """`ld_unet_forward` with `LD_FWD_PAIR` (the CFG pair of a sampler step: the layers in front of the first cross-attention evaluated once for both halves)
    against `ld_unet_forward` on cat([x, x]) — the same rows up to the rounding of tile / split choices that follow the row count — for the tiny
    net at B = 1 / 2 (two contexts per sample: the halves must differ) and, below, for the SD1.5 net against the reference golden."""
    g = load_golden("unet_tiny_16x16")
    gen = torch.Generator().manual_seed(5)
    for b in (1, 2):
        x = (torch.randn(b, 4, 16, 16, generator=gen) * 3.0).to(DEV)
        s = torch.tensor([2.5, 0.7][:b], device=DEV)
        ctx = torch.randn(2 * b, 77, g["ctx"].shape[-1], generator=gen)
        tiny_unet.set_context(ctx)
        full = tiny_unet.forward(torch.cat([x, x]).contiguous(), torch.cat([s, s]).contiguous()).cpu()
        pair = tiny_unet.forward_pair(x, s).cpu()
        assert pair.shape == full.shape and rel_l2(pair, full) < 1e-3, (b, rel_l2(pair, full))
        assert not torch.equal(pair[:b], pair[b:])                   # the cond half really saw the other context
        assert torch.equal(pair, tiny_unet.forward_pair(x, s).cpu())   # bitwise reproducible
        assert tiny_unet.last_launches > 0


def test_forward_pair_without_a_transformer_in_the_first_block():
    """A layout whose first input block has no SpatialTransformer (transformer_depth[0] = 0): the shared part of a CFG pair then ends at that
    block's output (the first cross-attention sits in a later block)."""
    from lightdiffusion_amd.unet import synthetic_unet
    cfg = dict(W.tiny_unet_config(), transformer_depth=[0, 1, 1, 1, 1, 1, 0, 0])
    u = synthetic_unet(cfg, max_batch=4, max_hw=(16, 16))
    gen = torch.Generator().manual_seed(6)
    x = (torch.randn(2, 4, 16, 12, generator=gen) * 3.0).to(DEV)
    s = torch.tensor([2.5, 0.7], device=DEV)
    u.set_context(torch.randn(4, 77, cfg["context_dim"], generator=gen))
    full = u.forward(torch.cat([x, x]).contiguous(), torch.cat([s, s]).contiguous()).cpu()
    pair = u.forward_pair(x, s).cpu()
    assert rel_l2(pair, full) < 1e-3 and not torch.equal(pair[:2], pair[2:])
    ctx = torch.randn(4, 77, cfg["context_dim"], generator=torch.Generator().manual_seed(7))
    u.set_context(ctx)
    pair = u.forward_pair(x, s).cpu()
    ref = O.apply_model(W.synth_state_dict(W.unet_param_shapes(cfg)), cfg, O.ModelSampling(), torch.cat([x, x]).cpu(), torch.cat([s, s]).cpu(), ctx)
    assert rel_l2(pair, ref) < UNET_TOL


def test_sd15_forward_pair_against_reference_golden():
    """SD1.5 net: the golden's two samples carry different x, so each is run as its own CFG pair (x_i twice, contexts [ctx_j, ctx_i]): the cond half
    of pair i must be the reference's denoised row i."""
    from lightdiffusion_amd.unet import synthetic_unet
    g = load_golden("unet_sd15_64x64")
    u = synthetic_unet(W.sd15_unet_config(), max_batch=2, max_hw=(64, 64))
    for i in (0, 1):
        u.set_context(torch.stack([g["ctx"][1 - i], g["ctx"][i]]))
        den = u.forward_pair(g["x"][i:i + 1].to(DEV).contiguous(), g["sigma"][i:i + 1].to(DEV).contiguous()).cpu()
        assert rel_l2(den[1], g["denoised"][i]) < UNET_TOL
    del u
    torch.cuda.empty_cache()


def test_wrapper_hook_contract(tiny_unet):
    """Drive the object exactly as calc_cond_batch does (LD.py:2558-2567) with the recorded hook arguments."""
    g = load_golden("samplers")
    params = {"input": g["hook_input"], "timestep": g["hook_timestep"],
              "c": {"c_crossattn": g["hook_ctx"], "transformer_options": {}}, "cond_or_uncond": g["hook_cond_or_uncond"].tolist()}
    out = tiny_unet(None, params)
    assert out.shape == g["hook_input"].shape and out.dtype == torch.float32
    cfg = W.tiny_unet_config()
    sd = W.synth_state_dict(W.unet_param_shapes(cfg))
    ref = O.apply_model(sd, cfg, O.ModelSampling(), g["hook_input"], g["hook_timestep"], g["hook_ctx"])
    assert rel_l2(out.cpu(), ref) < UNET_TOL
    assert tiny_unet.to("cuda:0") is tiny_unet
    out2 = tiny_unet(None, params)          # same context again: must hit the cached projections, same result
    assert torch.equal(out2, out)


def test_wrapper_hook_replays_graphs_bitwise_and_follows_the_prompt(tiny_unet):
    """the object on the reference's `model_function_wrapper` seam replays captured hipGraphs (the counterpart of
    StableFastPatch's enable_cuda_graph, LD.py:9896-9933).  [uncond, cond] batches of ONE latent take the CFG-pair graph, checked on the
    device; graph == eager bitwise on both routes; a second prompt of the same shape (recycled address or not) is not stale; halves that
    differ fall back to the plain graph within the same call."""
    g = load_golden("samplers")
    x, s, ctx = g["hook_input"].to(DEV), g["hook_timestep"].to(DEV), g["hook_ctx"].to(DEV)
    b = x.shape[0] // 2
    assert torch.equal(x[:b], x[b:]) and torch.equal(s[:b], s[b:])          # what calc_cond_batch recorded: cat([x_in, x_in])
    mk = lambda xx, cc: {"input": xx, "timestep": s, "c": {"c_crossattn": cc, "transformer_options": {"cond_or_uncond": [1, 0], "sigmas": s[:b]}},
                         "cond_or_uncond": [1, 0]}
    key = (x.shape[0], x.shape[2], x.shape[3])
    tiny_unet._hook.clear()
    out = tiny_unet(None, mk(x, ctx.clone()))
    run = tiny_unet._hook[key]
    assert run.pair.graph is not None and run.plain.graph is None and not run.halves_differed
    eager_pair = tiny_unet.forward_pair(x[:b].contiguous(), s[:b].contiguous())
    assert torch.equal(out, eager_pair)                                       # graph == eager, bit for bit
    cfg = W.tiny_unet_config()
    sd = W.synth_state_dict(W.unet_param_shapes(cfg))
    ms = O.ModelSampling()
    assert rel_l2(out.cpu(), O.apply_model(sd, cfg, ms, x.cpu(), s.cpu(), ctx.cpu())) < UNET_TOL
    # a second prompt of the same shape: the speculative replay is redone after the device-side check found the conditioning changed
    ctx2 = ctx + 0.5 * torch.randn(ctx.shape, generator=torch.Generator().manual_seed(5)).to(DEV)
    out_b = tiny_unet(None, mk(x, ctx2))
    assert rel_l2(out_b.cpu(), O.apply_model(sd, cfg, ms, x.cpu(), s.cpu(), ctx2.cpu())) < UNET_TOL
    assert not torch.equal(out_b, out)
    assert torch.equal(tiny_unet(None, mk(x, ctx2.clone())), out_b)           # same prompt again: cached projections, same bits
    assert torch.equal(tiny_unet(None, mk(x, ctx.clone())), out)              # and back to the first prompt
    # halves that are NOT the same latents: the call itself falls back to the plain graph, == the eager plain forward bit for bit
    x2 = x.clone()
    x2[b:] += 0.25
    out2 = tiny_unet(None, mk(x2, ctx.clone()))
    assert run.halves_differed and run.plain.graph is not None
    assert torch.equal(out2, tiny_unet.forward(x2, s))
    assert rel_l2(out2.cpu(), O.apply_model(sd, cfg, ms, x2.cpu(), s.cpu(), ctx.cpu())) < UNET_TOL
    # the reference calls the wrapper from a daemon worker thread under torch.inference_mode() (LD.py:10453, 10493): first contact there
    # (buffers, capture), then the same call from the main thread in normal mode — same bits both ways
    import threading
    tiny_unet._hook.clear()
    tiny_unet._ctx_ref = None
    box = {}

    def worker():
        try:
            with torch.inference_mode():
                box["out"] = tiny_unet(None, mk(x, ctx.clone())).clone()
        except Exception as e:      # noqa: BLE001 (re-raised on the main thread)
            box["err"] = e

    th = threading.Thread(target=worker, daemon=True)
    th.start()
    th.join()
    assert "err" not in box, box.get("err")
    assert torch.equal(box["out"], out) and torch.equal(tiny_unet(None, mk(x, ctx.clone())), out)
    # eager switch (A/B) and unload: .to("cpu") drops the captured graphs like the reference's graph-mode plugin does (LD.py:9921-9933)
    tiny_unet.hook_graph = False
    try:
        assert torch.equal(tiny_unet(None, mk(x2, ctx.clone())), out2)
    finally:
        tiny_unet.hook_graph = True
    assert tiny_unet.to(torch.device("cpu")) is tiny_unet and not tiny_unet._hook and not tiny_unet._denoisers


def test_sd15_unet_golden():
    from lightdiffusion_amd.unet import synthetic_unet
    g = load_golden("unet_sd15_64x64")
    u = synthetic_unet(W.sd15_unet_config(), max_batch=2, max_hw=(64, 64))
    u.set_context(g["ctx"])
    eps = u.forward(g["x"].to(DEV), g["sigma"].to(DEV), eps_only=True).cpu()
    den = u.forward(g["x"].to(DEV), g["sigma"].to(DEV)).cpu()
    assert rel_l2(eps, g["eps"]) < UNET_TOL and rel_l2(den, g["denoised"]) < UNET_TOL
    assert abs(u.last_flops / 2 - 803.3e9) / 803.3e9 < 0.03      # 803.3 GFLOP per UNet-eval
    del u
    torch.cuda.empty_cache()


def test_vae_tiny_golden():
    from lightdiffusion_amd.unet import synthetic_vae
    g = load_golden("vae_tiny")
    v = synthetic_vae(W.tiny_vae_config(), max_batch=1, max_hw=(8, 6))
    img = v.decode(g["z"])
    assert img.shape == g["img"].shape and img.device.type == "cpu"
    assert float((img - g["img"]).abs().max()) < 2.0 / 255.0 and float((img - g["img"]).abs().mean()) < 0.25 / 255.0


def test_vae_sd15_golden():
    from lightdiffusion_amd.unet import synthetic_vae
    g = load_golden("vae_sd15")
    v = synthetic_vae(W.sd15_vae_config(), max_batch=1, max_hw=(32, 32))
    img = v.decode(g["z"])
    assert img.shape == (1, 256, 256, 3)
    assert float((img[:, ::4, ::4] - g["img_sub"]).abs().max()) < 2.0 / 255.0
    assert abs(float(img.mean() - g["mean"])) < 1e-3


@pytest.mark.parametrize("tag,hw", [("tiny", (8, 6)), ("sd15", (32, 32))])
def test_vae_encode_golden(tag, hw):
    """VAE.encode: moments against the reference's Encoder + quant_conv; sample with the host generator."""
    from lightdiffusion_amd.unet import synthetic_vae
    g = load_golden("vae_enc_" + tag)
    cfg = W.tiny_vae_config() if tag == "tiny" else W.sd15_vae_config()
    v = synthetic_vae(cfg, max_batch=1, max_hw=hw, with_encoder=True)
    m = v.encode_moments(g["pixels"]).cpu()
    assert m.shape == g["moments"].shape
    assert rel_l2(m, g["moments"]) < 5e-3
    torch.manual_seed(58)
    z = v.encode(g["pixels"])
    assert z.device.type == "cpu" and rel_l2(z, g["z_seed58"]) < 5e-3
    img = v.decode(z)                                   # round trip through the decoder still works on the same handle
    assert img.shape == g["pixels"].shape and torch.isfinite(img).all()


def test_clip_text_model_on_hip_kernels():
    """the CLIP-L text transformer through the C ABI kernels vs the reference's CLIPTextModel golden
    (tiny config) and vs the pinned oracle at full CLIP-L size."""
    from lightdiffusion_amd.clip import CLIP, CLIPTextModelHIP
    g = load_golden("clip_tiny")
    cfg = W.tiny_clip_config()
    tm = CLIPTextModelHIP(cfg, W.synth_state_dict(W.clip_param_shapes(cfg)), device=DEV)
    last, inter, pooled = tm(g["tokens"], intermediate_output=-2)
    assert rel_l2(last.cpu(), g["last"]) < 5e-3 and rel_l2(inter.cpu(), g["inter_m2"]) < 5e-3 and rel_l2(pooled.cpu(), g["pooled"]) < 5e-3
    cond = CLIP(tm, None, layer_idx=-2).encode_from_tokens([[(t, 1.0) for t in g["tokens"][0].tolist()]])
    assert cond.shape == (1, 77, cfg["hidden_size"]) and cond.device.type == "cpu"
    cfg = W.sd15_clip_config()
    sd = W.synth_state_dict(W.clip_param_shapes(cfg))
    toks = g["tokens"][:1]
    ref = O.clip_text_model(sd, cfg, toks, layer_idx=-2)
    out = CLIPTextModelHIP(cfg, sd, device=DEV)(toks, intermediate_output=-2)[1].cpu()
    assert rel_l2(out, ref) < 5e-3
