"""CPU: the error-bound checker (tests/errbound.py) is sharp enough to catch the errors rel-L2 hides, and the route table of
tests/test_routes_gpu.py names every contraction kernel template the sources define."""
import math
import os
import re

import pytest
import torch

import errbound as EB
from conftest import ROOT


def _case(M=300, N=192, K=256, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g).half()
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).half()
    b = (torch.randn(N, generator=g) * 0.5).half()
    r = torch.randn(M, N, generator=g).half()
    ref, bound = EB.linear_ref(x, w, b, r)
    return x, w, b, r, ref, bound


def _rtz(ref):
    """fp16 rounding toward zero: RTN, then one step toward zero wherever RTN rounded away from zero."""
    y = ref.half()
    away = (y.double().abs() > ref.abs()) & (y != 0)
    bits = y.view(torch.int16).clone()
    bits[away] -= 1                    # sign-magnitude: one less magnitude step
    return bits.view(torch.float16)


def test_accepts_round_to_nearest_result():
    *_, ref, bound = _case()
    r, s = EB.check(ref.half(), ref, bound, "RTN")
    assert r <= 1.0 and abs(s) < 1e-5


def test_rejects_one_element_off_by_one_percent():
    *_, ref, bound = _case()
    y = ref.clone()
    y[171, 77] *= 1.01
    with pytest.raises(AssertionError, match=r"element bound: 1 of .*row 171, column 77.*tile \(1, 0\)"):
        EB.check(y.half(), ref, bound, "one element", tile=(128, 160))


def test_rejects_one_column_missing_its_bias():
    x, w, b, r, ref, bound = _case()
    y = ref.clone()
    y[:, 100] -= b[100].double()
    with pytest.raises(AssertionError, match=r"element bound: .*column 100"):
        EB.check(y.half(), ref, bound, "bias column")


def test_rejects_last_ragged_tile_without_residual():
    x, w, b, r, ref, bound = _case()
    y = ref.clone()
    y[256:] -= r[256:].double()                       # M = 300, 128-row tiles: the last tile holds rows 256..299
    with pytest.raises(AssertionError, match=r"element bound: .*tile \(2, "):
        EB.check(y.half(), ref, bound, "ragged tile", tile=(128, 160))


def test_rejects_round_toward_zero_by_the_bias_statistic():
    *_, ref, bound = _case(M=512, N=320)
    y = _rtz(ref)
    s = EB.signed_bias(y, ref)
    assert s < -EB.BIAS_TOL, s
    with pytest.raises(AssertionError, match="signed bias"):
        EB.check(y, ref, bound, "RTZ")


def test_rtn_bias_statistic_is_noise():
    *_, ref, _ = _case(M=512, N=320, seed=3)
    assert abs(EB.signed_bias(ref.half(), ref)) < EB.BIAS_TOL / 10


def _simulated_attention(q, k, v, heads, rtz):
    """The flash kernels' arithmetic without the ones column: fp32 scores from the fp16-rounded q * scale * log2(e), exp2 weights, P
    converted to fp16 (round to nearest or toward zero), numerator from the fp16 P, denominator from the unrounded fp32 weights."""
    b, lq, c = q.shape
    d = c // heads
    c2 = (1.0 / math.sqrt(d)) * 1.4426950408889634
    qs = (q.float() * c2).half().float().reshape(b, lq, heads, d).transpose(1, 2)
    kf = k.float().reshape(b, -1, heads, d).transpose(1, 2)
    vf = v.float().reshape(b, -1, heads, d).transpose(1, 2)
    s = qs @ kf.transpose(-1, -2)
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    ph = _rtz(p.double()) if rtz else p.half()
    o = (ph.float() @ vf) / p.sum(-1, keepdim=True)
    return o.half().transpose(1, 2).reshape(b, lq, c)


@pytest.mark.parametrize("d", [64, 160])
def test_attention_bound_accepts_rtn_and_rejects_truncated_p(d):
    g = torch.Generator().manual_seed(d)
    b, heads, lq, lk = 1, 2, 128, 256
    q, k, v = (torch.randn(b, n, heads * d, generator=g).half() for n in (lq, lk, lk))
    ref, bound = EB.attention_ref(q, k, v, heads)
    EB.check(_simulated_attention(q, k, v, heads, rtz=False), ref, bound, "RTN P")
    with pytest.raises(AssertionError, match="signed bias"):
        EB.check(_simulated_attention(q, k, v, heads, rtz=True), ref, bound, "RTZ P")
    ones = torch.ones_like(v)
    assert bool((_simulated_attention(q, k, ones, heads, rtz=False).float() == 1.0).all())
    assert float(_simulated_attention(q, k, ones, heads, rtz=True).float().max()) < 1.0


def test_cpu_conv_reference_matches_im2col():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 7, 5, 64, generator=g).half()
    wt = (torch.randn(32, 64, 3, 3, generator=g) / 24).half()
    for stride, out_hw in ((1, None), (2, None), (1, (11, 9)), (1, (14, 10))):
        ref, _, (ho, wo) = EB.conv_ref(x, wt, stride=stride, out_hw=out_hw)
        rows = EB.boundary_rows(ref.shape[0], 16, ho * wo, wo)
        cpu = EB.cpu_rows_conv(x, wt, rows, stride, out_hw)
        assert torch.allclose(cpu, ref[rows], rtol=1e-12, atol=1e-12), (stride, out_hw)


def test_every_contraction_kernel_template_has_a_route_row():
    """A new __global__ kernel in gemm.hip, a kernel family's source (gemm3.hip, gemm5.hip, conv6.hip, gemm7.hip, conv8.hip) or attention.hip
    cannot land without a pinned row in tests/test_routes_gpu.py
    (conv8_repack_kernel is the weight-layout copy behind conv8, not a contraction: it has no route of its own)."""
    import test_routes_gpu as R
    csrc = os.path.join(ROOT, "lightdiffusion_amd", "csrc")
    names = set()
    for f in ("gemm.hip", "gemm3.hip", "gemm5.hip", "conv6.hip", "gemm7.hip", "conv8.hip", "attention.hip"):
        names.update(re.findall(r"__global__\s+(?:__launch_bounds__\([^)]*\)\s+)?void\s+(\w+_kernel)\s*\(", open(os.path.join(csrc, f)).read()))
    names.discard("conv8_repack_kernel")
    assert {"gemm3_kernel", "gemm4_kernel", "gemm5_kernel", "conv6_kernel", "gemm7_kernel", "conv8_kernel", "splitk_reduce_kernel", "splitk_reduce_gn_kernel",
            "flash_attn2_kernel", "flash_attn512_kernel"} <= names
    pinned = {n.split("<")[0] for n in R.route_names()}
    assert not names - pinned, f"kernel templates without a route row: {sorted(names - pinned)}"
