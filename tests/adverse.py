"""Adverse statistics for the parity tests (helper module): a weight source that drives the synthetic networks to the activation range of a real
checkpoint, and deterministic operand profiles for the kernel-level tests.

Every element-wise test of the suite fed the kernels randn at scale 1.  All bounds of tests/errbound.py scale with the operands, so a correct kernel
passes at any magnitude; these inputs are where an fp16 store, a var = msq - mu^2 finished in fp32, a packed fp16 add onto a rounded tile or an
activation's tail would show if it were wrong.

source(model): weights.synth_tensor with
  * the weights of the convolutions / linears that write into the residual stream behind a normalisation or an attention (.conv2, .out_layers.3,
    .to_out.0, .ff.net.2) times GAIN[model], and every output row r of those with r % 37 == 5 another 16 (outlier channels);
  * with z the standardised synthetic draw, norm gains 2^(1.5 z) (about 0.04 .. 20) and norm biases 2 z;
  * all other biases times 20.  The factors on whole weight tensors and rows (GAIN and 16) are powers of two, so the fp16 rounding of a scaled
    weight is the scaled rounding.
The convolutions that are linear in the stream (upsample.conv, downsample.conv, .op, nin_shortcut, skip_connection, proj_out) keep their synthetic
scale: the same gain on them compounds to 1e8 and beyond.  GAIN is fixed by tests/test_adverse_cpu.py: the fp32 oracle's peak |activation| on the
tiny cases lies in [2^13, 2^15], a factor 2 below fp16's 65504.

source('clip'), the text model: the stream writers are self_attn.out_proj and mlp.fc2 (gain and x 16 rows as above), the norms layer_norm1 / 2 and
final_layer_norm, other biases x 20; the embedding tables keep their synthetic scale except position row 0, which is x 64 — every later query then
attends to an outlier key 0, so the causal attention sees peaked scores.  A stress profile: no checkpoint is available offline and none of these
figures measures one.  GAIN['clip'] and CHAIN_GAIN[('clip', *)] are fixed by tests/test_clip_chain_cpu.py::test_adverse_clip_window: the fp32
oracle's peak over the stages the product stores lies in [2^13, 2^15.5] (tiny x 64: 2.1e4; CLIP-L's width with 2 layers x 64: 1.8e4; the 12 layers
x 32: 1.7e4 — the stream grows with depth, so the deeper model takes the smaller gain).
"""
from __future__ import annotations

import math
import re

import torch

import chain_harness as H
from lightdiffusion_amd import weights as W

# one gain per model (a power of two).  Peaks of the fp32 oracle on fp16-rounded weights with these gains: tests/test_adverse_cpu.py::test_window
GAIN = {"unet": 16.0, "vae": 128.0, "clip": 32.0}
# the gain of the executor / chain tests (tests/test_adverse_chain_gpu.py) per (model, config).  Their window is asserted on the fp64 references of
# the stages the executor STORES, and the UNet executor never stores the oracle's hottest stage: ff.net.2 is folded into proj_out (mlp_out_fold).
# What it stores peaks well below the oracle's figure, so the window [2^13, 2^15.5] — which that test asserts per case, and whose peaks
# profiles/adverse_parity.json records — needs the next power of two for the tiny config and the one after for SD1.5.  At the tiny gain the fp32
# oracle's own peak, the unstored stage included, stays below 2^15.5 (tests/test_adverse_cpu.py::test_window_at_the_chain_gain); the SD1.5 oracle
# was not run on the CPU.
CHAIN_GAIN = {("unet", "tiny"): 32.0, ("unet", "sd15"): 64.0, ("vae", "tiny"): 128.0, ("vae", "fallback"): 128.0, ("vae", "sd15"): 128.0,
              ("clip", "tiny"): 64.0, ("clip", "w2"): 64.0, ("clip", "sd15"): 32.0}
OUTLIER_EVERY, OUTLIER_AT, OUTLIER_GAIN = 37, 5, 16.0
BIAS_GAIN = 20.0

_STREAM_WRITERS = re.compile(r"\.(conv2|out_layers\.3|to_out\.0|ff\.net\.2|self_attn\.out_proj|mlp\.fc2)\.weight$")
_NORM = re.compile(r"(^|\.)(norm\d?|norm_out|in_layers\.0|out_layers\.0|out\.0|layer_norm\d|final_layer_norm)\.(weight|bias)$")
POSITION_ROW0_GAIN = 64.0


def is_norm(name: str) -> bool:
    return _NORM.search(name) is not None


def source(model: str, seed: int = 0, gain: float | None = None):
    """A WeightSource (name, shape -> fp32 tensor) of the adverse network of `model` ('unet', 'vae' or 'clip')."""
    s = GAIN[model] if gain is None else gain

    def get(name, shape):
        t = W.synth_tensor(name, tuple(shape), seed)
        if name.endswith("embedding.weight"):             # the text model's tables: synthetic scale, but position row 0 (every later query attends
            if "position_embedding" in name:              # to an outlier key 0: the causal kernel sees peaked scores)
                t[0] = t[0] * POSITION_ROW0_GAIN
            return t
        if is_norm(name):
            if name.endswith(".weight"):
                return torch.exp2(1.5 * (t - 1.0) / 0.1)
            return 2.0 * (t / 0.05)
        if len(shape) == 1:
            return t * BIAS_GAIN
        if _STREAM_WRITERS.search(name):
            t = t * s
            rows = torch.arange(shape[0]) % OUTLIER_EVERY == OUTLIER_AT
            t[rows] = t[rows] * OUTLIER_GAIN
        return t
    return get


def state_dict(model: str, shapes, seed: int = 0, gain: float | None = None, fp16_rounded: bool = True):
    """The adverse state dict in fp32 (fp16_rounded: every value rounded through fp16 once, as a load stores it)."""
    src = source(model, seed, gain)
    sd = {k: src(k, v) for k, v in shapes.items()}
    return {k: v.half().float() for k, v in sd.items()} if fp16_rounded else sd


def record(case: str, what: dict) -> None:
    """With LD_WRITE_PARITY=1: merge `what` into the entry `case` of profiles/adverse_parity.json (a record, not an assertion)."""
    H.record("adverse_parity.json", case, what)


# ------------------------------------------------------------------ operand profiles (deterministic: shape and seed -> fp16)

def _randn(shape, seed):
    return torch.randn(tuple(shape), generator=torch.Generator().manual_seed(seed))


def big(shape, seed, device="cuda:0"):
    """randn * 2^10."""
    return (_randn(shape, seed) * 1024.0).half().to(device)


def mean(shape, seed, device="cuda:0", ratio=30.0, scale=16.0):
    """(randn + 30) * 2^4: mu / sigma = 30."""
    return ((_randn(shape, seed) + ratio) * scale).half().to(device)


def outlier(shape, seed, device="cuda:0"):
    """randn with every channel c % 37 == 5 and every row r % 53 == 7 times 64 (an element in both: times 64 once)."""
    x = _randn(shape, seed)
    x2 = x.reshape(-1, shape[-1])
    f = torch.ones_like(x2)
    f[:, torch.arange(shape[-1]) % 37 == 5] = 64.0
    f[torch.arange(x2.shape[0]) % 53 == 7, :] = 64.0
    return (x2 * f).reshape(x.shape).half().to(device)


def heavy(shape, seed, device="cuda:0"):
    """randn * exp2(2 randn): heavy tails, |x| from 1e-3 to a few hundred."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(tuple(shape), generator=g)
    return (a * torch.exp2(2.0 * torch.randn(tuple(shape), generator=g))).half().to(device)


PROFILES = {"big": big, "mean": mean, "outlier": outlier, "heavy": heavy}


def cancel(y_pre: torch.Tensor) -> torch.Tensor:
    """A residual that cancels 7/8 of the fp64 pre-residual reference: -y_pre (1 - 2^-3) rounded to fp16.  The packed fp16 adds round relative
    to |pre|, the result is |pre| / 8: their share of the error is eight times what it is against a randn residual."""
    return (-y_pre.double() * (1.0 - 2.0 ** -3)).half()


# the groups of groups(...): mu / sigma = +30, -30, a constant group (tests/test_norm_gpu.py::test_groupnorm_statistics_under_stress), and one group
# whose first channel is 64 times its other channels
G_POS, G_NEG, G_CONST, G_DOM = 3, 17, 9, 24


def groups(n, hw, c1, c2, seed, device="cuda:0"):
    """x [n][hw][C] split at c1, gamma, beta as tests/test_norm_gpu.py::gn_input builds them (a different mean and scale per group), with the four
    stress groups above.  -> (x1, x2 or None, gamma, beta) in fp16."""
    c = c1 + c2
    cpg = c // 32
    g = torch.Generator().manual_seed(seed)
    grp = torch.arange(c) // cpg
    off = (torch.arange(32).float() - 15.5) * 0.25
    sc = 0.5 + (torch.arange(32) % 5).float() * 0.3
    off[G_POS], off[G_NEG], sc[G_POS], sc[G_NEG] = 30.0, -30.0, 1.0, 1.0
    off[G_CONST], sc[G_CONST] = 2.75, 0.0
    x = torch.randn(n, hw, c, generator=g) * sc[grp] + off[grp]
    x[..., G_DOM * cpg] *= 64.0
    x = x.half().to(device)
    ga = (1.0 + 0.5 * torch.randn(c, generator=g)).half().to(device)
    be = (0.5 * torch.randn(c, generator=g)).half().to(device)
    return x[..., :c1].contiguous(), (x[..., c1:].contiguous() if c2 else None), ga, be


def group_bias(cout, seed, device="cuda:0", sigma=1.0):
    """A per-channel bias that puts a convolution's output of standard deviation `sigma` at mu / sigma = +30, -30 and +15 in three groups."""
    cpg = cout // 32
    b = _randn((cout,), seed) * 0.5
    grp = torch.arange(cout) // cpg
    b[grp == G_POS] = 30.0 * sigma
    b[grp == G_NEG] = -30.0 * sigma
    b[grp == G_DOM] = 15.0 * sigma
    return b.half().to(device)


# ------------------------------------------------------------------ operands of the linear and LayerNorm-fold rows

def linear_operands(profile, M, N, K, act, seed, dev="cuda:0"):
    """x in `profile`, w ~ N(0, 1 / K) (GEGLU: the value rows times 2^-10, so that value x gate stays in fp16's range), bias at the output's
    magnitude (the standard deviation of x w^T, rounded to a power of two)."""
    x = PROFILES[profile]((M, K), seed, dev)
    g = torch.Generator().manual_seed(seed + 1)
    w = torch.randn(N, K, generator=g) / math.sqrt(K)
    if act == "geglu":
        w[:N // 2] *= 2.0 ** -10
    w = w.half().to(dev)
    mag = 2.0 ** round(math.log2(float(x.float().pow(2).mean().sqrt()) + 1e-30))
    b = torch.randn(N, generator=g) * 0.5 * mag
    if act == "geglu":
        b[:N // 2] *= 2.0 ** -10
    return x, w, b.half().to(dev), mag


def ln_operands(M, C, N, ratio, scale, seed, dev="cuda:0"):
    """Operands of ops.linear_ln whose t = x wp^T + bp has mu / sigma = ratio at `scale` in every row: x randn * scale, wp ~ N(0, 1 / C),
    bp = ratio * scale (+ 0.2 scale randn)."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, sc=1.0, off=0.0: (torch.randn(*s, generator=g) * sc + off).half().to(dev)
    x, wp = r(M, C, sc=scale), r(C, C, sc=1 / math.sqrt(C))
    bp = r(C, sc=0.2 * scale, off=ratio * scale)
    gamma, beta = r(C, sc=0.2, off=1.0), r(C, sc=0.2)
    w, b = r(N, C, sc=1 / math.sqrt(C)), r(N, sc=0.2)
    return x, wp, bp, gamma, beta, w, b


LN_STATS = [(30.0, 16.0), (8.0, 128.0)]
