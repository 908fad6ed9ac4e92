"""CPU: regional conditioning (sampling.process_conds, sampling_function with model_options["ld_cond_areas"], the apply_cond_areas keyword, the
Conditioning* nodes) on a toy denoiser that logs the contexts and shapes it is called with; the two new ops run on their own host branches, the
samplers' device operators on their torch arithmetic (test_preview_cpu.host_update_arithmetic).
  * process_conds: percentage rounding, mask resize, mask bounds (the empty mask too), percent_to_sigma against the sigma table, same-area
    pairing in both directions, every ValueError; the caller's dicts are never modified;
  * grouping and accumulation order, and the result of sampling_function for a mixed set — a whole entry, two overlapping areas of different
    shapes, a fractional mask, strength 0.5 — BITWISE against tests/regional_ref.py (upstream's loops restated);
  * a step range keeps its entry out of the logged model calls on exactly the steps upstream would skip, at one host read of sigma per step;
  * NO BEHAVIOUR CHANGE: with the option off the same keyed lists give today's bits (today's expression restated here), and with the option on
    unkeyed single conditioning takes today's route."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import regional_ref as R                                                                   # noqa: E402
from test_preview_cpu import _ToyInner, _ToyPatcher, host_update_arithmetic                # noqa: E402,F401  (the fixture is used by name)
from lightdiffusion_amd import nodes as N                                                  # noqa: E402
from lightdiffusion_amd import ops                                                         # noqa: E402
from lightdiffusion_amd import sampling as S                                               # noqa: E402

B, H, W = 2, 16, 24
MS = S.ModelSampling()
same_bits = R.same_bits


def ctx(seed):
    """a context whose first element names it in the log"""
    t = torch.randn(1, 77, 8, generator=torch.Generator().manual_seed(seed))
    t[0, 0, 0] = float(seed)
    return t


def cond(seed, **keys):
    return [[ctx(seed), dict(keys)]]


class LoggingInner(_ToyInner):
    def __init__(self):
        self.calls = []

    def apply_model(self, x, t, c_crossattn=None, transformer_options=None, **kw):
        assert c_crossattn.shape[0] == x.shape[0] == t.shape[0], "one context row and one sigma per sample"
        self.calls.append((tuple(x.shape), [int(v) for v in c_crossattn[:, 0, 0].tolist()], list((transformer_options or {}).get("cond_or_uncond", []))))
        return super().apply_model(x, t, c_crossattn=c_crossattn)


def patcher():
    p = _ToyPatcher()
    p.model = LoggingInner()
    return p


def processed(pos, neg, b=B, h=H, w=W):
    return S.process_conds(S.convert_cond(pos), S.convert_cond(neg), (b, 4, h, w), torch.device("cpu"), MS)


def frac_mask(seed, *shape):
    return torch.randint(0, 65, shape, generator=torch.Generator().manual_seed(seed)).float() / 64.0


# ------------------------------------------------------------------ process_conds
def test_percent_to_sigma_against_the_table():
    assert MS.percent_to_sigma(0.0) == 999999999.9 and MS.percent_to_sigma(-1.0) == 999999999.9
    assert MS.percent_to_sigma(1.0) == 0.0 and MS.percent_to_sigma(2.0) == 0.0
    half = MS.percent_to_sigma(0.5)                                   # t = 499.5: halfway between two table entries in log sigma
    assert isinstance(half, float)
    want = (0.5 * MS.log_sigmas[499] + 0.5 * MS.log_sigmas[500]).exp()
    assert half == float(want) and float(MS.sigmas[499]) < half < float(MS.sigmas[500])
    assert MS.percent_to_sigma(0.25) > half > MS.percent_to_sigma(0.75)


def test_percentage_areas_round_as_upstream():
    pos, _ = processed(cond(1, area=("percentage", 0.5, 0.34, 0.26, 0.1)), cond(2))
    assert pos[0]["area"] == (8, round(0.34 * 24), round(0.26 * 16), round(0.1 * 24)) == (8, 8, 4, 2)
    pos, _ = processed(cond(1, area=("percentage", 0.3, 1.0, 0.0, 0.0)), cond(2), h=1)
    assert pos[0]["area"] == (1, 24, 0, 0), "round(0.3 * 1) is 0: a side is at least 1"
    pos, _ = processed(cond(1, area=(8, 12, 2, 4)), cond(2))
    assert pos[0]["area"] == (8, 12, 2, 4), "latent units are taken as they are"


def test_masks_are_resized_and_repeated():
    m = torch.rand(1, 128, 192, generator=torch.Generator().manual_seed(3))
    pos, _ = processed(cond(1, mask=m), cond(2))
    got = pos[0]["mask"]
    assert tuple(got.shape) == (1, H, W) and got.dtype == torch.float32 and got.is_contiguous()
    assert same_bits(got, F.interpolate(m.unsqueeze(1), size=(H, W), mode="bilinear", align_corners=False).squeeze(1))
    on_grid = torch.rand(H, W, generator=torch.Generator().manual_seed(4))
    assert same_bits(processed(cond(1, mask=on_grid), cond(2))[0][0]["mask"], on_grid[None]), "a mask on the latent grid is taken as it is"
    assert tuple(processed(cond(1, mask=torch.rand(B, H, W)), cond(2))[0][0]["mask"].shape) == (B, H, W)
    three = torch.rand(3, H, W, generator=torch.Generator().manual_seed(5))
    assert same_bits(processed(cond(1, mask=three), cond(2))[0][0]["mask"], three[:2]), "3 masks for a batch of 2: cut"
    pair = torch.rand(2, H, W, generator=torch.Generator().manual_seed(6))
    assert same_bits(processed(cond(1, mask=pair), cond(2), b=3)[0][0]["mask"], torch.cat([pair, pair[:1]])), "2 masks for a batch of 3: repeated and cut"
    assert same_bits(processed(cond(1, mask=pair.double()), cond(2))[0][0]["mask"], pair), "fp32 whatever came in"


def test_mask_bounds_become_the_area():
    m = torch.zeros(2, H, W)
    m[0, 3:14, 5:7] = 0.5                                             # rows 3..13, columns 5..6
    m[1, 2:4, 4:18] = -1.0                                            # rows 2..3, columns 4..17: the box is that of max_b |mask| > 0
    pos, neg = processed(cond(1, mask=m, set_area_to_bounds=True), cond(2))
    assert pos[0]["area"] == (12, 14, 2, 4)
    assert [c.get("area") for c in neg] == [None, (12, 14, 2, 4)], "and the negative list got its partner"
    thin = torch.zeros(H, W)
    thin[12:14, 20:22] = 1.0                                          # raised to 8 x 8, cut at the latent's edge: 16 - 12, 24 - 20
    masked_neg = cond(2, mask=torch.ones(H, W))                       # (its copy is the partner: masked, so the cut box needs no feather)
    assert processed(cond(1, mask=thin, set_area_to_bounds=True), masked_neg)[0][0]["area"] == (4, 4, 12, 20)
    with pytest.raises(ValueError, match="negative conditioning entry 1.*narrower than 8"):
        processed(cond(1, mask=thin, set_area_to_bounds=True), cond(2))                    # the partner, a copy of the unmasked negative, would feather
    thin = torch.zeros(H, W)
    thin[2:4, 3:5] = 1.0
    assert processed(cond(1, mask=thin, set_area_to_bounds=True), cond(2))[0][0]["area"] == (8, 8, 2, 3)
    assert processed(cond(1, mask=torch.zeros(H, W), set_area_to_bounds=True), cond(2))[0][0]["area"] == (8, 8, 0, 0), "the empty mask"
    assert processed(cond(1, mask=thin, set_area_to_bounds=False), cond(2))[0][0].get("area") is None
    big = torch.zeros(128, 192)
    big[64:, 96:] = 1.0                                               # resized first: the lower right quarter and its bilinear fringe
    area = processed(cond(1, mask=big, set_area_to_bounds=True), cond(2))[0][0]["area"]
    assert area == (8, 12, 8, 12)


def test_step_ranges_become_sigmas():
    pos, neg = processed(cond(1, start_percent=0.25, end_percent=0.75), cond(2, start_percent=0.0, end_percent=1.0))
    assert pos[0]["timestep_start"] == MS.percent_to_sigma(0.25) and pos[0]["timestep_end"] == MS.percent_to_sigma(0.75)
    assert neg[0]["timestep_start"] == 999999999.9 and neg[0]["timestep_end"] == 0.0
    assert "timestep_start" not in processed(cond(1), cond(2))[0][0]


def test_same_area_pairing_in_both_directions():
    a_small, a_big, a_other = (8, 8, 4, 4), (12, 16, 2, 2), (8, 8, 8, 16)
    pos = cond(1, area=a_small) + cond(2)
    neg = cond(3) + cond(4, area=a_big) + cond(5, area=(16, 24, 0, 0)) + cond(6, area=a_other)
    p, n = processed(pos, neg)
    name = lambda c: (int(c["cross_attn"][0, 0, 0]), c.get("area"))
    # positive -> negative: a_small lies in a_big (192) and in the whole-latent area (384): the smaller wins over the larger and over the entry
    # without an area; a copy of entry 4 with a_small is appended
    assert [name(c) for c in n] == [(3, None), (4, a_big), (5, (16, 24, 0, 0)), (6, a_other), (4, a_small)]
    # negative -> positive: a_big, the whole area and a_other are contained in no positive area: the positive entry without one is copied; a_small
    # finds itself
    assert [name(c) for c in p] == [(1, a_small), (2, None), (2, a_big), (2, (16, 24, 0, 0)), (2, a_other)]
    # an entry that already has exactly the area is not copied, and on a tie of h * w the earlier entry is taken
    p, n = processed(cond(1, area=a_small), cond(2, area=a_small) + cond(3))
    assert [name(c) for c in n] == [(2, a_small), (3, None)] and [name(c) for c in p] == [(1, a_small)]
    p, n = processed(cond(1, area=(8, 8, 4, 4)), cond(2, area=(8, 16, 4, 0)) + cond(3, area=(16, 8, 0, 4)))
    assert [name(c) for c in n][-1] == (2, (8, 8, 4, 4))
    # the copy keeps its source's other keys
    p, n = processed(cond(1, area=a_small, strength=0.5), cond(2, strength=2.0))
    assert n[1]["strength"] == 2.0 and n[1]["area"] == a_small and n[1]["cross_attn"] is n[0]["cross_attn"]


@pytest.mark.parametrize("keys,match", [
    (dict(area=(8, 8, 9, 0)), "leaves the"), (dict(area=(8, 8, 0, 17)), "leaves the"), (dict(area=(8, 8, -1, 0)), "leaves the"),
    (dict(area=("percentage", 0.5, 0.5, 0.75, 0.0)), "leaves the"),
    (dict(area=(0, 8, 0, 0)), "side < 1"), (dict(area=(8, -2, 0, 0)), "side < 1"),
    (dict(area=(4, 24, 2, 0)), "narrower than 8"), (dict(area=(16, 7, 0, 0)), "narrower than 8"), (dict(area=(16, 7, 0, 17)), "narrower than 8"),
    (dict(area=(8, 8, 0)), "area"), (dict(mask=torch.ones(1, 1, H, W)), "mask"),
])
def test_rejections(keys, match):
    with pytest.raises(ValueError, match=match):
        processed(cond(1, **keys), cond(2))
    with pytest.raises(ValueError, match=match):
        processed(cond(2), cond(1, **keys))


def test_narrow_areas_that_need_no_feather_are_accepted():
    processed(cond(1, area=(4, 24, 0, 0)), cond(2), h=4)                                # narrow, but every edge is the latent's
    processed(cond(1, area=(16, 7, 0, 0)), cond(2), w=7)
    processed(cond(1, area=(4, 4, 2, 2), mask=torch.ones(H, W)), cond(2, mask=torch.ones(H, W)))     # masked, and so is its partner: no feather at all


def test_more_than_sixteen_active_entries_are_refused():
    many = sum((cond(i) for i in range(1, 17)), [])
    assert len(processed(many[:15], cond(20))[0]) == 15
    with pytest.raises(ValueError, match="17 conditioning entries are active"):
        processed(many, cond(20))
    early = [[c[0], {"start_percent": 0.0, "end_percent": 0.4}] for c in many[:8]]
    late = [[c[0], {"start_percent": 0.6, "end_percent": 1.0}] for c in many[:15]]
    processed(early + late, cond(20))                                                    # 24 entries, but never more than 15 + 1 at once
    with pytest.raises(ValueError, match="active"):
        processed(early + [[c[0], {"start_percent": 0.3, "end_percent": 1.0}] for c in many[:9]], cond(20))      # 8 + 9 + 1 overlap


def test_process_conds_leaves_the_callers_dicts_alone():
    m = torch.rand(1, 32, 48)
    pos = cond(1, area=("percentage", 0.5, 0.5, 0.0, 0.0), strength=0.5) + cond(2, mask=m, set_area_to_bounds=True, start_percent=0.1, end_percent=0.9)
    neg = cond(3)
    before = [dict(c[1]) for c in pos + neg]
    cp, cn = S.convert_cond(pos), S.convert_cond(neg)
    snap = [dict(c) for c in cp + cn]
    p, n = S.process_conds(cp, cn, (B, 4, H, W), torch.device("cpu"), MS)
    assert [dict(c[1]) for c in pos + neg] == before and len(cp) == 2 and len(cn) == 1
    for c, s in zip(cp + cn, snap):
        assert c.keys() == s.keys() and all(c[k] is s[k] for k in s)
    assert p[0] is not cp[0] and p[1]["mask"] is not m and len(n) == 3


# ------------------------------------------------------------------ the step: grouping, accumulation order, the bits
A1, A2 = (12, 12, 0, 4), (12, 16, 4, 8)           # overlap rows 4..11, columns 8..15: both areas' ramps


def mixed():
    """a whole entry, two overlapping areas of different shapes (one at strength 0.5), a fractional mask; one negative"""
    pos = cond(1) + cond(2, area=A1, strength=1.0) + cond(3, area=A2, strength=0.5) + cond(4, mask=frac_mask(9, B, H, W), mask_strength=0.75)
    return processed(pos, cond(5))


def step_inputs(seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 4, H, W, generator=g) * 4.0, torch.full((B,), 2.5)


def test_groups_and_accumulation_order_and_the_bits_of_the_result():
    pos, neg = mixed()
    assert [c.get("area") for c in neg] == [None, A1, A2]
    x, sigma = step_inputs()
    inner = LoggingInner()
    opts = {"ld_cond_areas": True}
    got = S.sampling_function(inner, x, sigma, neg, pos, 7.5, opts)
    # [cond.., uncond..] = 1, 2@A1, 3@A2, 4, 5, 5@A1, 5@A2; shapes in the order they first appear: whole, A1's, A2's; reversed inside a group
    whole = (H, W, 0, 0)
    assert inner.calls == [((3 * B, 4, H, W), [5] * B + [4] * B + [1] * B, [1, 0, 0]),
                           ((2 * B, 4, 12, 12), [5] * B + [2] * B, [1, 0]),
                           ((2 * B, 4, 12, 16), [5] * B + [3] * B, [1, 0])]
    toy = _ToyInner()
    run = lambda windows, seeds: toy.apply_model(R.gather(x, windows), torch.cat([sigma] * len(windows)),
                                                 c_crossattn=torch.cat([ctx(s).expand(B, -1, -1) for s in seeds]))
    outs = [run([whole] * 3, [5, 4, 1]), run([A1] * 2, [5, 2]), run([A2] * 2, [5, 3])]
    E = ops.RegionalEntry
    table = [E(1, 0, 0, whole), E(0, 0, 1, whole, 1.0, pos[3]["mask"], 0.75), E(0, 0, 2, whole),
             E(1, 1, 0, A1), E(0, 1, 1, A1, 1.0),
             E(1, 2, 0, A2), E(0, 2, 1, A2, 0.5)]
    want = R.combine(outs, table, 7.5, (B, 4, H, W))
    assert torch.isfinite(want).all() and same_bits(got, want)
    # the order matters to the bits: accumulate the cond entries the other way round and some element differs
    other = R.combine(outs, [table[i] for i in (0, 6, 4, 2, 1, 3, 5)], 7.5, (B, 4, H, W))
    assert not same_bits(other, want) and torch.allclose(other, want, rtol=1e-4, atol=1e-4)
    # a second step of the same run reuses the plan: the same calls again, the same contexts
    inner.calls.clear()
    assert same_bits(S.sampling_function(inner, x, sigma, neg, pos, 7.5, opts), want) and len(inner.calls) == 3
    # and the keys are not inert: the option-off result on the same lists is another one
    assert not torch.allclose(S.sampling_function(LoggingInner(), x, sigma, neg, pos, 7.5, {}), want, atol=1e-3)


def test_a_model_function_wrapper_sees_each_group():
    pos, neg = mixed()
    x, sigma = step_inputs(1)
    seen = []

    def wrapper(apply_model, params):
        seen.append((tuple(params["input"].shape), params["cond_or_uncond"], params["c"]["transformer_options"]["ld_ctx_token"]))
        return apply_model(params["input"], params["timestep"], **params["c"])
    a = S.sampling_function(LoggingInner(), x, sigma, neg, pos, 3.0, {"ld_cond_areas": True, "model_function_wrapper": wrapper})
    b = S.sampling_function(LoggingInner(), x, sigma, neg, pos, 3.0, {"ld_cond_areas": True})
    assert same_bits(a, b) and [s[:2] for s in seen] == [((3 * B, 4, H, W), [1, 0, 0]), ((2 * B, 4, 12, 12), [1, 0]), ((2 * B, 4, 12, 16), [1, 0])]
    assert len({s[2] for s in seen}) == 3, "a context token per group"


def today(inner, x, sigma, neg, pos, scale):
    """the multi-entry route as it stands without the option, restated: every entry over the whole latent, averaged per list"""
    n_u, n_c = len(neg), len(pos)
    rows = lambda c: c["cross_attn"].expand(B, -1, -1)
    ctxs = torch.cat([rows(c) for c in reversed(neg)] + [rows(c) for c in reversed(pos)])
    out = inner.apply_model(torch.cat([x] * (n_u + n_c)), torch.cat([sigma] * (n_u + n_c)), c_crossattn=ctxs)
    parts = out.chunk(n_u + n_c)
    u = torch.stack(parts[:n_u]).sum(0) / float(n_u)
    c = torch.stack(parts[n_u:]).sum(0) / float(n_c)
    return u + (c - u) * scale


def test_option_off_is_todays_bits_for_keyed_lists():
    pos = S.convert_cond(cond(1) + cond(2, area=A1, strength=0.5) + cond(4, mask=frac_mask(9, B, H, W), start_percent=0.9, end_percent=1.0))
    neg = S.convert_cond(cond(5, area=("percentage", 0.5, 0.5, 0.0, 0.0)))
    x, sigma = step_inputs(2)
    for opts in ({}, {"ld_cond_areas": False}, None):
        inner = LoggingInner()
        got = S.sampling_function(inner, x, sigma, neg, pos, 7.5, opts)
        assert same_bits(got, today(_ToyInner(), x, sigma, neg, pos, 7.5))
        assert [c[0] for c in inner.calls] == [(4 * B, 4, H, W)], "one call on every entry over the whole latent"


def test_unkeyed_entries_with_the_option_are_the_plain_average_or_the_plain_route(host_update_arithmetic):
    x, sigma = step_inputs(3)
    # two unkeyed positives: the regional route, whose arithmetic gives today's bits ((a + b) / (1e-37 + 2) is (a + b) / 2)
    pos, neg = processed(cond(1) + cond(2), cond(5))
    inner = LoggingInner()
    got = S.sampling_function(inner, x, sigma, neg, pos, 7.5, {"ld_cond_areas": True})
    assert same_bits(got, today(_ToyInner(), x, sigma, neg, pos, 7.5)) and [c[:2] for c in inner.calls] == [((3 * B, 4, H, W), [5] * B + [2] * B + [1] * B)]
    # one unkeyed entry per list (strength 1 counts as no key): the existing route, here the un-fused call on [uncond, cond] and cfg_combine
    for keys in ({}, {"strength": 1.0}):
        pos, neg = processed(cond(1, **keys), cond(5))
        inner = LoggingInner()
        got = S.sampling_function(inner, x, sigma, neg, pos, 7.5, {"ld_cond_areas": True})
        off = S.sampling_function(LoggingInner(), x, sigma, neg, pos, 7.5, {})
        assert same_bits(got, off) and [c[:2] for c in inner.calls] == [((2 * B, 4, H, W), [5] * B + [1] * B)]


def test_the_plain_route_does_not_touch_the_new_ops(monkeypatch, host_update_arithmetic):
    boom = lambda *a, **k: (_ for _ in ()).throw(AssertionError("the plain route must not gather or combine"))
    monkeypatch.setattr(S.ops, "regional_gather", boom)
    monkeypatch.setattr(S.ops, "regional_combine", boom)
    x, sigma = step_inputs(4)
    pos, neg = processed(cond(1), cond(5))
    S.sampling_function(LoggingInner(), x, sigma, neg, pos, 7.5, {"ld_cond_areas": True})
    pos, neg = processed(cond(1, strength=0.5), cond(5))
    with pytest.raises(AssertionError, match="plain route"):
        S.sampling_function(LoggingInner(), x, sigma, neg, pos, 7.5, {"ld_cond_areas": True})


# ------------------------------------------------------------------ whole runs: the keyword, step ranges, the host read
STEPS = 4


def run(pos, neg, sampler="euler_ancestral", model=None, **kw):
    model = patcher() if model is None else model
    lat = {"samples": torch.randn(B, 4, H, W, generator=torch.Generator().manual_seed(7))}
    torch.manual_seed(3)                                                                  # euler_ancestral draws on the global generator
    out = S.common_ksampler(model, 5, STEPS, 3.0, sampler, "normal", pos, neg, lat, **kw)[0]["samples"]
    return out, model.model.calls


@pytest.mark.parametrize("sampler", ["euler_ancestral", "dpmpp_2m_sde"])
def test_a_step_range_skips_its_entry_on_the_steps_upstream_skips(host_update_arithmetic, monkeypatch, sampler):
    sigmas = S.calculate_sigmas(MS, "normal", STEPS)
    reads = []
    host_sigma = S._host_sigma
    monkeypatch.setattr(S, "_host_sigma", lambda t: (reads.append(1), host_sigma(t))[1])
    pos = cond(1) + cond(2, area=A1, start_percent=0.2, end_percent=0.7)
    neg = cond(5)
    ts_start, ts_end = MS.percent_to_sigma(0.2), MS.percent_to_sigma(0.7)
    on = [not (float(s) > ts_start or float(s) < ts_end) for s in sigmas[:-1]]         # upstream's comparison, on the step's sigma
    assert True in on and False in on, f"the range splits the schedule: {[float(s) for s in sigmas]} against ({ts_start}, {ts_end})"
    out, calls = run(pos, neg, sampler, apply_cond_areas=True)
    expected = []
    for active in on:
        if active:        # [1, 2@A1, 5, 5@A1]: the whole group [5, 1], then A1's group [5, 2]
            expected += [((2 * B, 4, H, W), [5] * B + [1] * B, [1, 0]), ((2 * B, 4, 12, 12), [5] * B + [2] * B, [1, 0])]
        else:             # 2@A1 and its partner 5@A1 ... the partner carries no range of its own: it stays, alone in its group
            expected += [((2 * B, 4, H, W), [5] * B + [1] * B, [1, 0]), ((B, 4, 12, 12), [5] * B, [1])]
    assert calls == expected
    assert len(reads) == STEPS, "one host read of sigma per step"
    assert torch.isfinite(out).all()
    reads.clear()
    run(cond(1) + cond(2, area=A1), neg, sampler, apply_cond_areas=True)
    assert reads == [], "no entry carries a range: sigma is never read"


def test_a_range_that_leaves_one_unkeyed_entry_per_list_takes_the_plain_route(host_update_arithmetic):
    sigmas = S.calculate_sigmas(MS, "normal", STEPS)
    pos = cond(1) + cond(2, mask=frac_mask(2, H, W), start_percent=0.5, end_percent=1.0)
    ts = MS.percent_to_sigma(0.5)
    late = [float(s) <= ts for s in sigmas[:-1]]
    assert True in late and False in late
    _, calls = run(pos, cond(5), apply_cond_areas=True)
    assert [c[1] for c in calls] == [[5] * B + [2] * B + [1] * B if l else [5] * B + [1] * B for l in late]


@pytest.mark.parametrize("sampler", ["euler_ancestral", "dpmpp_2m_sde", "dpm_adaptive"])
def test_the_keyword_reaches_the_sampler_and_off_nothing_changes(host_update_arithmetic, sampler):
    pos = cond(1) + cond(2, area=A1, strength=0.5)
    neg = cond(5)
    off, calls_off = run(pos, neg, sampler)
    assert all(c[0] == (3 * B, 4, H, W) for c in calls_off)
    # today's trajectory: the same lists without their keys
    plain, _ = run(cond(1) + cond(2), neg, sampler)
    assert same_bits(off, plain)
    assert same_bits(run(pos, neg, sampler, apply_cond_areas=False)[0], off)
    on, calls_on = run(pos, neg, sampler, apply_cond_areas=True)
    assert torch.isfinite(on).all() and not torch.equal(on, off) and any(c[0] == (2 * B, 4, 12, 12) for c in calls_on)
    # through the node, and composed with the noise mask: the kept half is the latent (euler_ancestral's last step to sigma = 0 is exact here)
    model = patcher()
    lat = {"samples": torch.randn(B, 4, H, W, generator=torch.Generator().manual_seed(7))}
    torch.manual_seed(3)
    node = N.KSampler2().sample(model, 5, STEPS, 3.0, sampler, "normal", pos, neg, lat, apply_cond_areas=True)[0]["samples"]
    assert same_bits(node, on)
    assert "ld_cond_areas" not in model.model_options, "the option lives on the run's copy of the options"


def test_with_the_noise_mask_as_well_the_kept_half_is_the_latent(host_update_arithmetic):
    pos = cond(1) + cond(2, area=A1, strength=0.5)
    L = torch.randn(B, 4, H, W, generator=torch.Generator().manual_seed(7))
    m = torch.ones(H, W)
    m[:, :12] = 0.0
    lat = N.SetLatentNoiseMask().set_mask({"samples": L}, m)[0]
    torch.manual_seed(3)
    out = N.KSampler2().sample(patcher(), 5, STEPS, 3.0, "dpmpp_2m_sde", "normal", pos, cond(5), lat, apply_noise_mask=True, apply_cond_areas=True)[0]["samples"]
    assert same_bits(out[..., :12], L[..., :12]) and float((out - L)[..., 12:].abs().mean()) > 0.05


def test_run_leaves_the_callers_conditioning_alone(host_update_arithmetic):
    m = frac_mask(2, 32, 48)
    pos = cond(1) + cond(2, mask=m, set_area_to_bounds=True, mask_strength=0.5, start_percent=0.0, end_percent=0.8)
    neg = cond(5)
    before = [(c[0].clone(), dict(c[1])) for c in pos + neg]
    run(pos, neg, apply_cond_areas=True)
    assert len(pos) == 2 and len(neg) == 1
    for (t, d), c in zip(before, pos + neg):
        assert torch.equal(t, c[0]) and d.keys() == c[1].keys() and all(d[k] is c[1][k] for k in d)


# ------------------------------------------------------------------ the nodes
def test_conditioning_nodes_build_new_lists():
    base = cond(1, pooled_output=None) + cond(2)
    snap = [dict(c[1]) for c in base]
    (a,) = N.ConditioningSetArea().append(base, 128, 64, 32, 16, 0.5)
    assert [c[1]["area"] for c in a] == [(8, 16, 2, 4)] * 2 and a[0][1]["strength"] == 0.5 and a[0][1]["set_area_to_bounds"] is False
    (p,) = N.ConditioningSetAreaPercentage().append(base, 0.5, 0.25, 0.1, 0.2, 1.5)
    assert p[0][1]["area"] == ("percentage", 0.25, 0.5, 0.2, 0.1) and p[0][1]["strength"] == 1.5 and p[0][1]["set_area_to_bounds"] is False
    m2 = torch.rand(64, 96)
    (m,) = N.ConditioningSetMask().append(base, m2, "mask bounds", 0.75)
    assert tuple(m[0][1]["mask"].shape) == (1, 64, 96) and m[0][1]["mask_strength"] == 0.75 and m[0][1]["set_area_to_bounds"] is True
    (d,) = N.ConditioningSetMask().append(base, torch.rand(2, 64, 96), "default", 1.0)
    assert tuple(d[1][1]["mask"].shape) == (2, 64, 96) and d[1][1]["set_area_to_bounds"] is False
    with pytest.raises(ValueError, match="set_cond_area"):
        N.ConditioningSetMask().append(base, m2, "bounds", 1.0)
    (r,) = N.ConditioningSetTimestepRange().set_range(base, 0.25, 0.75)
    assert r[0][1]["start_percent"] == 0.25 and r[1][1]["end_percent"] == 0.75
    (c,) = N.ConditioningCombine().combine(a, r)
    assert len(c) == 4 and c[0] is a[0] and c[3] is r[1] and len(a) == 2 and len(r) == 2
    for out in (a, p, m, d, r):
        assert out is not base and all(o[0] is b[0] and o[1] is not b[1] for o, b in zip(out, base)), "new lists, new dicts, the same tensors"
    assert [dict(c[1]) for c in base] == snap and a[0][1]["pooled_output"] is None, "the inputs are untouched, their other keys carried along"
