"""CPU control of tests/chain_harness.py: the chain tests of five executors stand or fall with it, so each of its checks is shown to accept
what is right and to reject one planted defect, by name.  Hand-made taps, tensors of a few dozen elements."""
import json
import os

import pytest
import torch

import chain_harness as H
import errbound as EB

TAPS = [dict(kind="first", name="conv_in", launches="k_in"), dict(kind="conv", name="block.0", launches="k_stats;k_conv", kernel="k_conv"),
        dict(kind="last", name="conv_out", launches="k_out")]
TABLE = ["k_in", "k_stats", "k_conv", "k_out"]


# ------------------------------------------------------------------ B1

def test_same_launches_accepts_the_matching_list():
    assert H.same_launches("case", TAPS, TABLE) == [("conv_in", "k_in"), ("block.0", "k_stats"), ("block.0", "k_conv"), ("conv_out", "k_out")]


def test_same_launches_rejects():
    with pytest.raises(AssertionError, match=r"case: launch 2 differs at block\.0: the chain ran k_conv, the executor k_other"):
        H.same_launches("case", TAPS, TABLE[:2] + ["k_other"] + TABLE[3:])
    with pytest.raises(AssertionError, match=r"the chain has 4 launches, the executor 3; first unmatched: \('conv_out', 'k_out'\)"):
        H.same_launches("case", TAPS, TABLE[:3])                     # a launch the executor does not have
    with pytest.raises(AssertionError, match=r"the chain has 4 launches, the executor 5; first unmatched: k_more"):
        H.same_launches("case", TAPS, TABLE + ["k_more"])            # a launch the chain does not have
    with pytest.raises(AssertionError, match=r"taps without a launch: \['idle'\]"):
        H.same_launches("case", TAPS + [dict(kind="conv", name="idle", launches="")], TABLE)


# ------------------------------------------------------------------ B2

def _flipped(t, index=(1, 2)):
    """t with the lowest mantissa bit of one element flipped."""
    bits = t.clone().view(torch.int32)
    bits[index] ^= 1
    return bits.view(torch.float32)


def test_same_bits():
    want = torch.arange(24, dtype=torch.float32).reshape(4, 6) + 0.5
    ran = []

    def run(case):
        ran.append(case)
        return want.clone()
    H.same_bits("A", want, run, ["B", "C"])
    assert ran == ["A", "B", "A", "C", "A"]
    with pytest.raises(AssertionError, match=r"^A: 1 of 24 elements differ, first at \[1, 2\]: executor 8\.5"):
        H.same_bits("A", want, lambda case: _flipped(want), ["B"])
    ran.clear()

    def stale(case):                                                 # the handle is right until another shape has run on it
        ran.append(case)
        return _flipped(want, (3, 5)) if "B" in ran else want.clone()
    with pytest.raises(AssertionError, match=r"^A after B: 1 of 24 elements differ, first at \[3, 5\]"):
        H.same_bits("A", want, stale, ["B"])
    ran.clear()
    H.same_bits("A", want, stale)                                    # (without a case in between there is nothing to see)
    image = torch.arange(12, dtype=torch.uint8).reshape(2, 6)
    H.same_bits("A", (want, image), lambda case: (want.clone(), image.clone()))
    with pytest.raises(AssertionError, match=r"^A, result 1: 1 of 12 elements differ, first at \[0, 4\]: executor 5\.0, chain 4\.0"):
        H.same_bits("A", (want, image), lambda case: (want.clone(), image + (torch.arange(12).reshape(2, 6) == 4)))
    with pytest.raises(AssertionError, match=r"A: shape \(6, 4\), the chain's \(4, 6\)"):
        H.bits_held(want.t(), want, "A")


# ------------------------------------------------------------------ B3

def _operands(seed=0, shape=(4, 8)):
    ref = torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    return ref.half(), ref, EB.U * ref.abs() + EB.TINY


def test_every_stage_reports_the_failed_stage_and_keeps_the_others():
    seen = []

    def stage(tap, what):
        seen.append(what)
        y, ref, bound = _operands()
        return [H.held(y * 1.01 if tap["kind"] == "conv" else y, ref, bound, what)]
    rec, fails = H.every_stage("case", TAPS, stage)
    assert seen == ["case conv_in [k_in]", "case block.0 [k_conv]", "case conv_out [k_out]"]
    assert len(fails) == 1 and fails[0].startswith("case block.0 [k_conv]: element bound: "), fails
    assert sorted(rec) == ["first", "last"] and all(sorted(v) == ["signed_bias_over_tolerance", "worst_error_over_bound"] for v in rec.values())
    assert all(0.0 < v["worst_error_over_bound"] <= 1.0 for v in rec.values()), rec
    with pytest.raises(AssertionError, match=r"^1 of 3 stages outside their bound:\ncase block\.0 \[k_conv\]: element bound"):
        H.stages_held(fails, TAPS)
    H.stages_held([], TAPS)
    # the worst figures per kind: the larger ratio, the signed bias of the larger magnitude with its sign, in units of BIAS_TOL
    pairs = {"conv_in": [(0.25, 1e-5), (0.5, -3e-5)], "block.0": [(0.125, 2e-5)], "conv_out": [(0.75, -1e-5)]}
    rec, fails = H.every_stage("case", TAPS + [dict(kind="first", name="conv_out", launches="k")], lambda tap, what: pairs[tap["name"]])
    assert not fails and rec == {"first": {"worst_error_over_bound": 0.75, "signed_bias_over_tolerance": round(-3e-5 / EB.BIAS_TOL, 4)},
                                 "conv": {"worst_error_over_bound": 0.125, "signed_bias_over_tolerance": round(2e-5 / EB.BIAS_TOL, 4)},
                                 "last": {"worst_error_over_bound": 0.75, "signed_bias_over_tolerance": round(-1e-5 / EB.BIAS_TOL, 4)}}


def _image_tap(n=5, rows=3, c=8, bad=None):
    """A tap of n images in the three layouts a chain hands over — [n][h][w][C], the rows [n L][C] of a linear, [n][C] — with an output pair;
    bad: (image, factor) scales that image's first output."""
    ref, bound = _operands(3, (n, rows, 1, c))[1:]
    y = ref.half()
    if bad is not None:
        y[bad[0]] *= bad[1]
    return dict(kind="conv", name="block.0", launches="k_conv", kernel="k_conv", n=n, par=dict(w=torch.arange(n)),
                inp=dict(x=ref, rows=ref.reshape(n * rows, c), rowvec=ref[:, 0, 0], stride=1, out_hw=(rows, 1), none=None),
                out=(y, y.reshape(n * rows, c)), part=torch.arange(n * 4.0).reshape(n, 2, 2))


def test_tap_images_cuts_every_layout_by_image():
    tap = _image_tap()
    cut = H.tap_images(tap, (0, -1))
    assert cut["n"] == 2 and cut["kind"] == "conv" and cut["par"] is tap["par"]                 # (parameters are shared: 5 weights stay 5)
    for k, full in (("x", tap["inp"]["x"]), ("rowvec", tap["inp"]["rowvec"])):
        assert torch.equal(cut["inp"][k], full[[0, 4]])
    assert torch.equal(cut["inp"]["rows"], tap["inp"]["x"][[0, 4]].reshape(6, 8))
    assert cut["inp"]["stride"] == 1 and cut["inp"]["out_hw"] == (3, 1) and cut["inp"]["none"] is None
    assert torch.equal(cut["out"][0], tap["out"][0][[0, 4]]) and torch.equal(cut["out"][1], tap["out"][1].reshape(5, 3, 8)[[0, 4]].reshape(6, 8))
    assert torch.equal(cut["part"], tap["part"][[0, 4]])
    assert H.image_indices((0, -1), 5) == [0, 4] and H.image_indices((0, -1), 1) == [0] and H.image_indices(H.EVERY_IMAGE, 3) == [0, 1, 2]
    with pytest.raises(AssertionError, match=r"image subset \(0, 7\) of a tap of 5 images"):
        H.tap_images(tap, (0, 7))
    with pytest.raises(AssertionError, match=r"block\.0: a tensor of shape \(7, 8\) in a tap of 5 images"):
        H.tap_images(dict(tap, inp=dict(x=torch.zeros(7, 8))), (0,))


def test_every_stage_on_an_image_subset():
    """The subset is a condition of the case table, not coverage: a defect in an image inside it is rejected by name, one in an image
    outside it is NOT SEEN by B3 (B2 still compares every image's bits with the chain's) — by construction."""
    whole = dict(kind="first", name="conv_in", launches="k_in", inp=dict(x=torch.zeros(5, 2)), par={}, out=torch.zeros(5, 2))
    seen = []

    def stage(tap, what):
        seen.append((what, tap.get("n"), tuple(tap["out"][0].shape) if "n" in tap else tuple(tap["out"].shape)))
        if "n" not in tap:
            return [(0.0, 0.0)]
        ref, bound = _operands(3, (5, 3, 1, 8))[1:]
        if " image " in what:                                            # (the reference of that one image, from the image the message names)
            j = int(what.rsplit(" ", 1)[1])
            ref, bound = ref[j:j + 1], bound[j:j + 1]
        return [H.held(tap["out"][0], ref, bound, what)]
    tap0 = _image_tap()
    rec, fails = H.every_stage("case", [whole, tap0], stage, images=(0, -1))
    assert not fails and sorted(rec) == ["conv", "first"]
    assert seen == [("case conv_in [k_in]", None, (5, 2)), ("case block.0 [k_conv] image 0", 1, (1, 3, 1, 8)), ("case block.0 [k_conv] image 4", 1, (1, 3, 1, 8))]
    tap0 = _image_tap(bad=(4, 1.01))                                     # inside the subset
    rec, fails = H.every_stage("case", [whole, tap0], stage, images=(0, -1))
    assert len(fails) == 1 and fails[0].startswith("case block.0 [k_conv] image 4: element bound: "), fails
    tap0 = _image_tap(bad=(2, 1.01))                                     # outside the subset: not seen ...
    rec, fails = H.every_stage("case", [whole, tap0], stage, images=(0, -1))
    assert not fails
    rec, fails = H.every_stage("case", [whole, tap0], stage, images=H.EVERY_IMAGE)            # ... seen with every image, one at a time
    assert len(fails) == 1 and fails[0].startswith("case block.0 [k_conv] image 2: element bound: "), fails
    seen.clear()
    H.every_stage("case", [whole, _image_tap()], stage)                  # no subset: the tap whole, as it was
    assert seen[1] == ("case block.0 [k_conv]", 5, (5, 3, 1, 8))


def test_partials_held():
    y = torch.randn(1, 2, 2, 64, generator=torch.Generator().manual_seed(1)).half()          # 4 pixels, 32 groups of 2 channels
    yg = y.double().reshape(1, 4, 32, 2)
    chunk = lambda rows: torch.stack([yg[:, rows].sum((1, 3)), (yg[:, rows] ** 2).sum((1, 3))], -1)
    part = torch.stack([chunk(slice(0, 1)), chunk(slice(1, 4))], 1).float()                   # [n][2 chunks][32 groups][sum, sum of squares]
    H.partials_held(part, y, "conv")
    part[0, 1, 5, 0] += 1e-3                                                                  # (the tolerance of a sum is below 1e-5 here)
    with pytest.raises(AssertionError, match=r"^conv: partial statistics, error / tolerance "):
        H.partials_held(part, y, "conv")


def test_held_goes_through_the_module_attribute_check(monkeypatch):
    calls = []
    monkeypatch.setattr(EB, "check", lambda y, ref, bound, what, **kw: calls.append((what, kw)) or "verdict")
    y, ref, bound = _operands()
    assert H.held(y, ref, bound, "small", bias_extra=0.5, image_rows=4, width=2) == "verdict"
    big = torch.ones(10 ** 4, dtype=torch.float64)
    assert H.held(big.half(), big, big, "big", bias_extra=0.5) == "verdict"
    assert calls == [("small", dict(bias_extra=0.5 + EB.rtn_noise(EB.independent_roundings(ref)), keep=None, image_rows=4, width=2)),
                     ("big", dict(bias_extra=0.5, keep=None))]


# ------------------------------------------------------------------ the record

def test_record(monkeypatch, tmp_path):
    monkeypatch.setattr(H, "PROFILES", str(tmp_path))
    monkeypatch.delenv("LD_WRITE_PARITY", raising=False)
    H.record("x_parity.json", "case", {"b": 2})
    monkeypatch.setenv("LD_WRITE_PARITY", "0")
    H.record("x_parity.json", "case", {"b": 2})
    assert os.listdir(tmp_path) == []
    monkeypatch.setenv("LD_WRITE_PARITY", "1")
    (tmp_path / "x_parity.json").write_text(json.dumps({"case": {"a": 1, "b": 0}, "other": {"z": 0}}))
    H.record("x_parity.json", "case", {"b": 2})
    H.record("x_parity.json", "new", {"c": 3})
    assert (tmp_path / "x_parity.json").read_text() == '{\n "case": {\n  "a": 1,\n  "b": 2\n },\n "new": {\n  "c": 3\n },\n "other": {\n  "z": 0\n }\n}\n'


# ------------------------------------------------------------------ the ControlNet chain tests' own stages and launch cost record

def test_control_add_stage_rejects_the_wrong_residual_sample():
    """tests/test_controlnet_chain_gpu.py `_stage`, kind control_add: sample s reads residual s % r_n — a residual read as s // r_n, the strength
    left out, or a sum rounded twice is named by its segment."""
    import test_controlnet_chain_gpu as T
    g = torch.Generator().manual_seed(3)
    t0, t1 = torch.randn(4, 2, 3, 8, generator=g).half(), torch.randn(4, 5, generator=g).half()
    r0, r1 = torch.randn(2, 2, 3, 8, generator=g).half(), torch.randn(2, 5, generator=g).half()
    good = lambda t, r, s=0.6: (t.float() + s * r.float().repeat((2,) + (1,) * (r.dim() - 1))).half()
    tap = dict(kind="control_add", name="control", inp=dict(t=[t0, t1], r=[r0, r1]), par=dict(strength=0.6, r_n=2), out=(good(t0, r0), good(t1, r1)))
    assert T._stage(tap, None, "case") == [(0.0, 0.0)]
    wrong_sample = (t1.float() + 0.6 * r1.float().repeat_interleave(2, 0)).half()
    for bad, segment in (((good(t0, r0), wrong_sample), 1), ((good(t0, r0, 1.0), good(t1, r1)), 0),
                         (((t0 + (0.6 * r0.float()).half().repeat(2, 1, 1, 1)), good(t1, r1)), 0)):
        with pytest.raises(AssertionError, match=rf"^case: segment {segment}: \d+ of \d+ elements differ"):
            T._stage(dict(tap, out=bad), None, "case")


def test_cost_of_sums_a_launch_table():
    import test_controlnet_chain_gpu as T
    rows = [("conv1", (8, 320, 320, 1), 0.0, 10.0, "a"), ("conv1", (8, 320, 320, 1), 0.0, 2.5, "b"), ("", (0, 0, 0, 0), 0.0, 1.25, "a")]
    assert T.cost_of(rows) == {"launches": 3, "us": 13.8, "per_kernel": {"a": [2, 11.2], "b": [1, 2.5]}}
