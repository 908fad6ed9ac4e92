"""GPU: the lifecycle the four resident models share (UNet, VAE, ESRGAN, TAESD), pinned at the C ABI: what a null handle, a handle
without weights, one without a workspace, a bad argument and a shape beyond the reserved workspace return; how the workspace size follows
`reserve`; what a profiled run leaves in the launch table; and the wrappers' lazy re-reserve, `reserve_epoch` and `__del__`.

Smallest models (the tiny UNet / VAE configurations, an RRDBNet of one block, TAESD), 8 x 8 latents or images, batch 1-2, synthetic
weights.  The statuses are exact.  Two counts follow the executors, not a guess: a GroupNorm that runs its statistics and its apply
kernel is ONE record of the launch table and TWO launches of `last_launches`, so the table of the UNet and the VAE is no longer than
`last_launches` (equal for ESRGAN and TAESD, whose records are one kernel each), and the UNet's per-class launch counts sum to it.
FLOPs are integer-valued doubles far below 2^53, so `last_flops` equals the sum of the table's column exactly.
"""
import ctypes as C

import pytest
import torch

from lightdiffusion_amd import weights as W
from lightdiffusion_amd._lib import ERR_ARG, ERR_SHAPE, ERR_STATE, F32, FWD_EPS_ONLY, FWD_PAIR, OK, ESRGANConfig, UNetConfig, VAEConfig, lib

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 123.0


def stream():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


class Family:
    """One resident model at the C ABI.  `dims(b, h, w)`: the arguments of reserve; `buffers`: (inputs, outputs) of the run entry point."""
    name = ""
    has_plan_bytes = True

    def fn(self, op):
        return getattr(lib(), f"ld_{self.name}_{op}")

    def dims(self, b, h, w):
        return (b, h, w)

    def reserve(self, hd, b, h, w):
        return self.fn("reserve")(hd, *self.dims(b, h, w))

    def ready(self, hd, b):
        """What a loaded, reserved handle still needs before a run of batch b (the UNet: its context)."""

    def run(self, hd, ins, outs, b, h, w, profile=False):
        return self.fn("profile" if profile else self.entry)(hd, *ins, *outs, b, h, w, stream())

    def null_runs(self):
        i, o = self.buffers(1, 8, 8)
        args = [ptr(t) for t in i + o]
        return {self.entry: self.fn(self.entry)(None, *args, 1, 8, 8, stream()), "profile": self.fn("profile")(None, *args, 1, 8, 8, stream())}


class UNet(Family):
    name, entry, has_plan_bytes = "unet", "forward", False

    def create(self):
        cfg, c = W.tiny_unet_config(), UNetConfig()
        c.in_channels, c.out_channels, c.model_channels = cfg["in_channels"], cfg["out_channels"], cfg["model_channels"]
        c.num_levels = len(cfg["channel_mult"])
        for k in ("channel_mult", "num_res_blocks", "transformer_depth", "transformer_depth_output"):
            for i, v in enumerate(cfg[k]):
                getattr(c, k)[i] = v
        c.transformer_depth_middle, c.context_dim, c.num_heads = cfg["transformer_depth_middle"], cfg["context_dim"], cfg["num_heads"]
        hd = C.c_void_p()
        return lib().ld_unet_create(C.byref(c), C.byref(hd)), hd

    def dims(self, b, h, w):
        return (b, h, w, 77)

    def ready(self, hd, b):
        ctx = torch.randn(b, 77, 64, generator=torch.Generator().manual_seed(3)).to(DEV)
        assert lib().ld_unet_set_context(hd, ctx.data_ptr(), F32, b, 77, stream()) == OK

    def buffers(self, b, h, w):
        g = torch.Generator().manual_seed(1)
        return [torch.randn(b, 4, h, w, generator=g).to(DEV), torch.ones(b, device=DEV)], [torch.full((b, 4, h, w), SENTINEL, device=DEV)]

    def run(self, hd, ins, outs, b, h, w, profile=False):
        if not profile:
            return lib().ld_unet_forward(hd, *ins, *outs, b, h, w, 0, None, stream())
        ms, fl, self.class_launches = (C.c_double * 6)(), (C.c_double * 6)(), (C.c_int * 6)()
        return lib().ld_unet_profile(hd, *ins, *outs, b, h, w, 0, None, stream(), ms, fl, self.class_launches)

    def null_runs(self):
        i, o = self.buffers(2, 8, 8)
        x, s, y = (t.data_ptr() for t in i + o)
        ms, fl, nl = (C.c_double * 6)(), (C.c_double * 6)(), (C.c_int * 6)()
        L = lib()
        return {"forward": L.ld_unet_forward(None, x, s, y, 2, 8, 8, 0, None, stream()),
                "forward_pair": L.ld_unet_forward(None, x, s, y, 1, 8, 8, FWD_PAIR, None, stream()),
                "profile": L.ld_unet_profile(None, x, s, y, 2, 8, 8, 0, None, stream(), ms, fl, nl),
                "profile_pair": L.ld_unet_profile(None, x, s, y, 1, 8, 8, FWD_PAIR, None, stream(), ms, fl, nl),
                "set_context": L.ld_unet_set_context(None, x, F32, 1, 77, stream())}


class VAE(Family):
    name, entry = "vae", "decode"

    def create(self, with_encoder=True):
        cfg, c = W.tiny_vae_config(), VAEConfig()
        c.with_encoder = int(with_encoder)
        c.z_channels, c.ch, c.num_levels = cfg["z_channels"], cfg["ch"], len(cfg["ch_mult"])
        for i, v in enumerate(cfg["ch_mult"]):
            c.ch_mult[i] = v
        c.num_res_blocks, c.out_ch = cfg["num_res_blocks"], cfg["out_ch"]
        hd = C.c_void_p()
        return lib().ld_vae_create(C.byref(c), C.byref(hd)), hd

    def buffers(self, b, h, w):
        g = torch.Generator().manual_seed(1)
        return [torch.randn(b, 4, h, w, generator=g).to(DEV)], [torch.full((b, 8 * h, 8 * w, 3), SENTINEL, device=DEV)]

    def encode_buffers(self, b, h, w):
        g = torch.Generator().manual_seed(2)
        return [torch.rand(b, 3, 8 * h, 8 * w, generator=g).to(DEV) * 2 - 1], [torch.full((b, 8, h, w), SENTINEL, device=DEV)]

    def null_runs(self):
        out = Family.null_runs(self)
        i, o = self.encode_buffers(1, 8, 8)
        out["encode"] = lib().ld_vae_encode(None, i[0].data_ptr(), o[0].data_ptr(), 1, 8, 8, stream())
        return out


class ESRGAN(Family):
    name, entry = "esrgan", "forward"

    def create(self):
        cfg, c = W.esrgan_config(nb=1), ESRGANConfig()
        c.in_nc, c.out_nc, c.nf, c.gc, c.nb, c.scale = (cfg[k] for k in ("in_nc", "out_nc", "nf", "gc", "nb", "scale"))
        hd = C.c_void_p()
        return lib().ld_esrgan_create(C.byref(c), C.byref(hd)), hd

    def buffers(self, b, h, w):
        g = torch.Generator().manual_seed(1)
        return [torch.rand(b, h, w, 3, generator=g).to(DEV)], [torch.full((b, 4 * h, 4 * w, 3), SENTINEL, device=DEV)]


class TAESD(Family):
    name, entry = "taesd", "decode"

    def create(self):
        hd = C.c_void_p()
        return lib().ld_taesd_create(C.byref(hd)), hd

    def buffers(self, b, h, w):
        g = torch.Generator().manual_seed(1)
        return ([torch.randn(b, h, w, 4, generator=g).to(DEV)],
                [torch.full((b, 8 * h, 8 * w, 3), SENTINEL, device=DEV), torch.full((b, 8 * h, 8 * w, 3), int(SENTINEL), dtype=torch.uint8, device=DEV)])


FAMILIES = {f.name: f for f in (UNet(), VAE(), ESRGAN(), TAESD())}
_weights = {}


def params(fam, hd):
    """[(name, shape)] of a handle, through param_count / param_info."""
    name, ndim, shape = C.c_char_p(), C.c_int(), (C.c_int64 * 4)()
    out = []
    for i in range(fam.fn("param_count")(hd)):
        assert fam.fn("param_info")(hd, i, C.byref(name), C.byref(ndim), shape) == OK
        out.append((name.value.decode(), tuple(int(shape[k]) for k in range(ndim.value))))
    return out


def load(fam, hd):
    """Every parameter of the handle from synthetic weights (made once per family, kept on the device)."""
    cache = _weights.setdefault(fam.name, {})
    for name, shape in params(fam, hd):
        if name not in cache:
            cache[name] = W.synth_tensor(name, shape).to(DEV).contiguous()
        assert fam.fn("load_param")(hd, name.encode(), cache[name].data_ptr(), F32, stream()) == OK, name
    torch.cuda.synchronize()


@pytest.fixture
def make():
    """make(fam, loaded, reserved shape or None, **create arguments) -> handle; every handle is destroyed behind the test."""
    made = []

    def _make(fam, loaded=False, reserved=None, **kw):
        st, hd = fam.create(**kw)
        assert st == OK and hd.value
        made.append((fam, hd))
        if loaded:
            load(fam, hd)
        if reserved is not None:
            assert fam.reserve(hd, *reserved) == OK
            if loaded:
                fam.ready(hd, reserved[0])
        return hd

    yield _make
    torch.cuda.synchronize()
    for fam, hd in made:
        fam.fn("destroy")(hd)


def untouched(outs):
    torch.cuda.synchronize()
    return all(bool((t == SENTINEL).all()) for t in outs)


families = pytest.mark.parametrize("fam", list(FAMILIES.values()), ids=list(FAMILIES))


@families
def test_null_handle(fam):
    for op in ("param_count", "workspace_bytes", "last_launches", "last_flops"):
        assert fam.fn(op)(None) == 0, op
    if fam.has_plan_bytes:
        assert fam.fn("plan_bytes")(None, 1, 8, 8) == 0
    name, ndim, shape = C.c_char_p(), C.c_int(), (C.c_int64 * 4)()
    w = torch.zeros(64, device=DEV)
    buf = C.create_string_buffer(4096)
    assert fam.fn("param_info")(None, 0, C.byref(name), C.byref(ndim), shape) == ERR_ARG
    assert fam.fn("load_param")(None, b"x", w.data_ptr(), F32, stream()) == ERR_ARG
    assert fam.reserve(None, 1, 8, 8) == ERR_ARG
    assert fam.fn("profile_launches")(None, buf, len(buf)) == ERR_ARG
    for entry, st in fam.null_runs().items():
        assert st == ERR_ARG, (entry, st)
    fam.fn("destroy")(None)


@families
def test_param_info_bounds_and_reserve_arguments(fam, make):
    hd = make(fam)
    n = fam.fn("param_count")(hd)
    name, ndim, shape = C.c_char_p(), C.c_int(), (C.c_int64 * 4)()
    assert n > 0 and len(params(fam, hd)) == n
    for i in (-1, n):
        assert fam.fn("param_info")(hd, i, C.byref(name), C.byref(ndim), shape) == ERR_ARG, i
    assert fam.fn("load_param")(hd, None, None, F32, stream()) == ERR_ARG
    dims = fam.dims(1, 8, 8)
    for k in range(len(dims)):
        assert fam.fn("reserve")(hd, *(0 if j == k else d for j, d in enumerate(dims))) == ERR_ARG, k
    assert fam.fn("workspace_bytes")(hd) == 0


@families
def test_workspace_follows_reserve(fam, make):
    hd = make(fam, reserved=(1, 8, 8))                          # (planning and reserving need no weights)
    ws = fam.fn("workspace_bytes")(hd)
    assert ws > 0
    if fam.has_plan_bytes:
        assert fam.fn("plan_bytes")(hd, 1, 8, 8) == ws
        assert fam.fn("plan_bytes")(hd, 0, 8, 8) == 0
        assert fam.fn("workspace_bytes")(hd) == ws              # a plan query reserves nothing
    assert fam.reserve(hd, 1, 8, 8) == OK
    assert fam.fn("workspace_bytes")(hd) == ws
    assert fam.reserve(hd, 2, 8, 8) == OK
    ws2 = fam.fn("workspace_bytes")(hd)
    assert ws2 > ws
    if fam.has_plan_bytes:
        assert fam.fn("plan_bytes")(hd, 2, 8, 8) == ws2


@families
def test_run_needs_weights_and_a_workspace(fam, make):
    ins, outs = fam.buffers(1, 8, 8)
    i, o = [ptr(t) for t in ins], [ptr(t) for t in outs]
    no_weights = make(fam, reserved=(1, 8, 8))
    assert fam.run(no_weights, i, o, 1, 8, 8) == ERR_STATE
    no_workspace = make(fam, loaded=True)
    assert fam.run(no_workspace, i, o, 1, 8, 8) == ERR_STATE
    assert untouched(outs)


@families
def test_run_statuses_at_a_reserved_shape(fam, make):
    hd = make(fam, loaded=True, reserved=(1, 8, 8))
    ins, outs = fam.buffers(2, 8, 8)
    i, o = [ptr(t) for t in ins], [ptr(t) for t in outs]
    assert fam.run(hd, [None] + i[1:], o, 1, 8, 8) == ERR_ARG
    assert fam.run(hd, i, [None] + o[1:], 1, 8, 8) == ERR_ARG
    assert fam.run(hd, i, o, 0, 8, 8) == ERR_SHAPE
    # a batch of 2 on a workspace reserved for 1 (the UNet: more samples than reserved, and not the context's): refused, nothing launched
    assert fam.run(hd, i, o, 2, 8, 8) == ERR_SHAPE
    assert untouched(outs)
    assert fam.run(hd, i, o, 1, 8, 8) == OK                     # the handle is still usable after the refused calls
    assert not untouched(outs)
    assert fam.reserve(hd, 2, 8, 8) == OK
    fam.ready(hd, 2)
    assert fam.run(hd, i, o, 2, 8, 8) == OK
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t.float()).all()) for t in outs)
    assert fam.fn("last_launches")(hd) > 0 and fam.fn("last_flops")(hd) > 0


@families
def test_profile_fills_the_launch_table(fam, make):
    hd = make(fam, loaded=True, reserved=(1, 8, 8))
    ins, outs = fam.buffers(1, 8, 8)
    buf = C.create_string_buffer(1 << 18)
    assert fam.fn("profile_launches")(hd, buf, len(buf)) == OK and buf.value == b""      # nothing profiled yet
    assert fam.run(hd, [ptr(t) for t in ins], [ptr(t) for t in outs], 1, 8, 8, profile=True) == OK
    assert fam.fn("profile_launches")(hd, buf, len(buf)) == OK
    rows = [line.split("\t") for line in buf.value.decode().splitlines()]
    launches, flops = fam.fn("last_launches")(hd), fam.fn("last_flops")(hd)
    print(f"{fam.name}: {len(rows)} records, last_launches {launches}, last_flops {flops:.0f}")
    assert all(len(r) == 8 for r in rows)
    assert 0 < len(rows) <= launches
    if fam.name in ("esrgan", "taesd"):
        assert len(rows) == launches
    if fam.name == "unet":
        assert sum(fam.class_launches) == launches
    assert sum(float(r[5]) for r in rows) == flops > 0
    assert fam.fn("profile_launches")(hd, buf, 8) == ERR_ARG    # a buffer too small for the table
    assert fam.fn("profile_launches")(hd, None, 0) == ERR_ARG


def test_forward_flags_are_checked_before_anything_is_launched():
    """The flags of ld_unet_forward / ld_unet_profile and ld_controlnet_forward / ld_controlnet_profile on valid handles with their context
    set: a bit that is no flag, eps of a pair and eps of a control branch are LD_ERR_ARG, a pair of no samples is LD_ERR_SHAPE — on the host:
    nothing is launched (last_launches stays) and nothing is written."""
    from lightdiffusion_amd.controlnet import synthetic_controlnet
    from lightdiffusion_amd.unet import synthetic_unet
    cfg = W.tiny_unet_config()
    unet = synthetic_unet(cfg, max_batch=2, max_hw=(8, 8), max_tokens=77)
    cnet = synthetic_controlnet(cfg, max_batch=2, max_hw=(8, 8), max_tokens=77)
    ctx = torch.randn(2, 77, cfg["context_dim"], generator=torch.Generator().manual_seed(3))
    unet.set_context(ctx)
    cnet.set_context(ctx)
    (x, s), (out,) = FAMILIES["unet"].buffers(2, 8, 8)
    ms, fl, nl = (C.c_double * 6)(), (C.c_double * 6)(), (C.c_int * 6)()
    L = lib()
    forms = {
        "ld_unet_forward": lambda n, flags: L.ld_unet_forward(unet._h, ptr(x), ptr(s), ptr(out), n, 8, 8, flags, None, stream()),
        "ld_unet_profile": lambda n, flags: L.ld_unet_profile(unet._h, ptr(x), ptr(s), ptr(out), n, 8, 8, flags, None, stream(), ms, fl, nl),
        "ld_controlnet_forward": lambda n, flags: L.ld_controlnet_forward(cnet._h, ptr(x), ptr(s), n, 8, 8, flags, stream()),
        "ld_controlnet_profile": lambda n, flags: L.ld_controlnet_profile(cnet._h, ptr(x), ptr(s), n, 8, 8, flags, stream()),
    }
    before = (unet.last_launches, cnet.last_launches)
    for name, call in forms.items():
        assert call(2, 4) == ERR_ARG, name
        assert call(1, FWD_PAIR | FWD_EPS_ONLY) == ERR_ARG, name
        assert call(0, FWD_PAIR) == ERR_SHAPE, name
        if "controlnet" in name:
            assert call(2, FWD_EPS_ONLY) == ERR_ARG, name
    assert (unet.last_launches, cnet.last_launches) == before
    assert untouched([out])


def test_vae_encode_needs_the_encoder(make):
    fam = FAMILIES["vae"]
    hd = make(fam, loaded=True, reserved=(1, 8, 8), with_encoder=False)
    ins, outs = fam.encode_buffers(1, 8, 8)
    assert lib().ld_vae_encode(hd, ins[0].data_ptr(), outs[0].data_ptr(), 1, 8, 8, stream()) == ERR_STATE
    assert untouched(outs)
    with_enc = make(fam, loaded=True, reserved=(1, 8, 8))
    assert lib().ld_vae_encode(with_enc, ins[0].data_ptr(), outs[0].data_ptr(), 1, 8, 8, stream()) == OK
    assert not untouched(outs)


def _wrappers():
    from lightdiffusion_amd.preview import MI355XTAESD
    from lightdiffusion_amd.unet import synthetic_unet, synthetic_vae
    from lightdiffusion_amd.upscale import MI355XUpscaler
    synth = lambda name, shape: W.synth_tensor(name, shape)   # noqa: E731
    z = torch.randn(2, 4, 8, 8, generator=torch.Generator().manual_seed(4))
    return {
        "unet": (lambda: synthetic_unet(W.tiny_unet_config(), max_batch=1, max_hw=(8, 8)), lambda m, b: m.set_context(torch.zeros(b, 77, 64))),
        "vae": (lambda: synthetic_vae(W.tiny_vae_config(), max_batch=1, max_hw=(8, 8)), lambda m, b: m.decode_device(z[:b])),
        "esrgan": (lambda: MI355XUpscaler(W.esrgan_config(nb=1), synth, max_batch=1, max_hw=(8, 8)), lambda m, b: m.forward_device(torch.rand(b, 8, 8, 3))),
        "taesd": (lambda: MI355XTAESD(synth, max_batch=1, max_hw=(8, 8)), lambda m, b: m.decode(z[:b])),
    }


@pytest.mark.parametrize("name", list(FAMILIES))
def test_wrapper_grows_the_workspace_and_dies_once(name):
    build, call = _wrappers()[name]
    m = build()
    ws, epoch = m.workspace_bytes, getattr(m, "reserve_epoch", None)
    assert ws > 0 and tuple(m._reserved[:3]) == (1, 8, 8)
    call(m, 1)                                                  # inside the plan: the workspace stays
    assert m.workspace_bytes == ws and getattr(m, "reserve_epoch", None) == epoch
    call(m, 2)                                                  # a larger call re-reserves
    assert tuple(m._reserved[:3]) == (2, 8, 8) and m.workspace_bytes > ws
    if name in ("unet", "taesd"):
        assert m.reserve_epoch == epoch + 1
    m._ensure(*m._reserved)                                     # the reserved shape again, and a smaller one: nothing moves
    m._ensure(*((1,) + tuple(m._reserved[1:])))
    assert tuple(m._reserved[:3]) == (2, 8, 8) and getattr(m, "reserve_epoch", None) == (None if epoch is None else epoch + 1)
    torch.cuda.synchronize()
    m.__del__()
    assert not m._h.value
    m.__del__()
