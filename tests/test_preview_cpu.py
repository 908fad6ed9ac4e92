"""CPU: the host side of the TAESD latent preview: tests/taesd_ref.py against the reference's TAESD (tests/golden/taesd_*.npz), the
decoder's key / shape list and file handling, LatentPreviewer's scheduling on a stand-in decoder, and the callback plumbing from
KSampler2 / common_ksampler down to the sampler loop on a toy denoiser."""
import pytest
import torch

import taesd_ref as TR
from conftest import load_golden, rel_l2
from lightdiffusion_amd import nodes as N
from lightdiffusion_amd import preview as P
from lightdiffusion_amd import sampling as S
from lightdiffusion_amd import weights as W

FIXTURES = ["taesd_9x13", "taesd_b2_17x33"]


def state_dict(seed=0):
    return {k: W.synth_tensor("taesd_decoder." + k, s, seed) for k, s in W.taesd_decoder_param_shapes().items()}


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_reproduces_the_reference(name):
    g = load_golden(name)
    y = TR.decode(state_dict(int(g["weight_seed"])), g["x"])
    assert y.shape == g["y"].shape and y.shape[1:3] == (8 * g["x"].shape[2], 8 * g["x"].shape[3])
    err = rel_l2(y, g["y"])
    print(f"{name}: rel-L2 {err:.3e}")
    assert err <= 1e-5
    assert torch.equal(TR.to_image(g["y"]), g["image"])


def test_param_shapes_are_the_reference_decoders_state_dict():
    shapes = W.taesd_decoder_param_shapes()
    assert len(shapes) == 67
    for name in FIXTURES:
        g = load_golden(name)
        want = [(str(k), tuple(int(d) for d in s if d)) for k, s in zip(g["keys"], g["shapes"].tolist())]
        assert list(shapes.items()) == want


def test_safetensors_file_loads_back_through_the_key_handling(tmp_path):
    from safetensors.torch import save_file
    sd = state_dict(3)
    bare = tmp_path / "taesd_decoder.safetensors"
    save_file(sd, str(bare))
    whole = tmp_path / "taesd.safetensors"                   # a whole TAESD module: prefixed decoder, the two scalars, encoder keys
    save_file({**{"taesd_decoder." + k: v for k, v in sd.items()}, "vae_shift": torch.tensor(0.0), "vae_scale": torch.tensor(1.0),
               "taesd_encoder.0.weight": torch.zeros(64, 3, 3, 3)}, str(whole))
    for path in (bare, whole):
        got = P.load_decoder_file(path)
        assert list(got) == list(sd) or set(got) == set(sd)
        assert all(torch.equal(got[k], sd[k]) for k in sd)
    with pytest.raises(KeyError):
        P.decoder_state_dict({k: v for k, v in sd.items() if k != "19.bias"})


class StandInDecoder:
    """image(latent) on the host: the batch row's first value in every byte, so that a test reads which rows of which tensor were decoded."""
    device = torch.device("cpu")

    def __init__(self):
        self.seen = []

    def image(self, lat):
        self.seen.append(lat.clone())
        b, _, h, w = lat.shape
        return lat[:, 0, 0, 0].to(torch.uint8).view(b, 1, 1, 1).expand(b, 8 * h, 8 * w, 3).contiguous()


def _steps(n, denoised=True):
    for i in range(n):
        x = torch.full((3, 4, 2, 3), 0.0) + torch.arange(3.0).view(3, 1, 1, 1) + 10 * i
        yield {"x": x, "i": i, "sigma": 1.0, "denoised": (x + 100) if denoised else None}


def test_previewer_honours_every_rows_and_source():
    got = []
    on = lambda i, im: got.append((i, im))
    p = P.LatentPreviewer(StandInDecoder(), on, use_graph=False)
    for d in _steps(4):
        p(d)
    assert [i for i, _ in got] == [0, 1, 2, 3]
    assert all(im.dtype == torch.uint8 and tuple(im.shape) == (1, 16, 24, 3) and im.device.type == "cpu" for _, im in got)
    assert [int(im[0, 0, 0, 0]) for _, im in got] == [0, 10, 20, 30]                       # row 0 of x

    got.clear()
    p = P.LatentPreviewer(StandInDecoder(), on, rows=slice(1, 3), every=2, use_graph=False)
    for d in _steps(5):
        p(d)
    assert [i for i, _ in got] == [1, 3]                                                     # every 2nd call
    assert [tuple(im.shape) for _, im in got] == [(2, 16, 24, 3)] * 2
    assert [im[:, 0, 0, 0].tolist() for _, im in got] == [[11, 12], [31, 32]]
    p.reset()
    p(next(_steps(1)))
    assert len(got) == 2                                                                     # the count starts again

    got.clear()
    p = P.LatentPreviewer(StandInDecoder(), on, source="denoised", use_graph=False)
    for d in _steps(2):
        p(d)
    assert [int(im[0, 0, 0, 0]) for _, im in got] == [100, 110]
    got.clear()
    for d in _steps(2, denoised=False):                                                      # dpm_adaptive has no denoised: x
        p(d)
    assert [int(im[0, 0, 0, 0]) for _, im in got] == [0, 10]
    with pytest.raises(ValueError):
        P.LatentPreviewer(StandInDecoder(), on, source="eps")
    with pytest.raises(ValueError):
        P.LatentPreviewer(StandInDecoder(), on, every=0)


class _ToyInner:
    """What CFGGuider and KSAMPLER touch of BaseModel: a denoiser x / (1 + sigma^2) shifted by the conditioning."""
    model_sampling = S.ModelSampling()

    def apply_model(self, x, t, c_crossattn=None, **kw):
        return x * (1.0 / (1.0 + t.view(-1, 1, 1, 1) ** 2)) + 0.01 * c_crossattn.mean(dim=(1, 2)).view(-1, 1, 1, 1)

    def process_latent_in(self, latent):
        return latent

    def process_latent_out(self, latent):
        return latent


class _ToyPatcher:
    load_device = torch.device("cpu")

    def __init__(self):
        self.model, self.model_options = _ToyInner(), {}

    def get_model_object(self, name):
        return getattr(self.model, name)


@pytest.fixture
def host_update_arithmetic(monkeypatch):
    """The samplers' fused updates are device operators; on the host the same arithmetic in torch."""
    def axpby_(x, a, y=None, b=0.0, z=None, c=0.0):
        x.mul_(a)
        if y is not None:
            x.add_(y, alpha=b)
        if z is not None:
            x.add_(z, alpha=c)
        return x

    def cfg_combine(den2, cfg):
        u, c = den2.chunk(2)
        return u + (c - u) * cfg
    monkeypatch.setattr(S.ops, "axpby_", axpby_)
    monkeypatch.setattr(S.ops, "cfg_combine", cfg_combine)


@pytest.mark.parametrize("sampler", ["euler_ancestral", "dpmpp_2m_sde"])
def test_ksampler_reaches_the_callback_once_per_step(host_update_arithmetic, sampler):
    cond = lambda s: [[torch.randn(1, 77, 8, generator=torch.Generator().manual_seed(s)), {}]]
    lat = {"samples": torch.zeros(2, 4, 3, 5)}
    args = (_ToyPatcher(), 5, 4, 3.0, sampler, "normal", cond(1), cond(2), lat)
    seen = []
    out = S.common_ksampler(*args, callback=lambda d: seen.append((d["i"], tuple(d["x"].shape), d["denoised"] is not None)))[0]["samples"]
    assert seen == [(i, (2, 4, 3, 5), True) for i in range(4)]
    assert torch.equal(out, S.common_ksampler(*args)[0]["samples"])                          # the callback is read-only

    dec, got = StandInDecoder(), []
    pv = P.LatentPreviewer(dec, lambda i, im: got.append((i, im)), every=2, use_graph=False)
    pv.calls = 1                                                                              # a previewer that has been used before
    out2 = N.KSampler2().sample(*args, preview=pv)[0]["samples"]
    assert torch.equal(out2, out)
    assert [i for i, _ in got] == [1, 3] and all(tuple(im.shape) == (1, 24, 40, 3) for _, im in got)
    assert all(tuple(l.shape) == (1, 4, 3, 5) for l in dec.seen)
