"""CPU: tools/inpaint_cost.py rehearsed without a device — its arguments, the alternation of the trees over the rounds, and the figures it derives
from canned child output (medians, the masked routes' differences to the unmasked one and to the parent's, the blend pair).  The measurement
itself needs the GPU; the child refuses to run without one."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import inpaint_cost as T      # noqa: E402


def canned(unmasked, masked, masked_dd, pair):
    return {"steps_ms": {"1": {"unmasked": list(unmasked), "masked": list(masked), "masked_dd": list(masked_dd)}}, "blend_pair_us": {"1": pair}}


def test_arguments():
    a = T.parse([])
    assert (a.steps, a.repeats, a.rounds, a.batches, a.parent_tree, a.child) == (30, 5, 2, [1, 8], None, False)
    assert a.out == os.path.join(ROOT, "profiles", "inpaint_cost.json") and a.package_root == ROOT
    a = T.parse(["--parent-tree", "/x", "--batches", "2", "--rounds", "3", "--child", "--variants", "unmasked"])
    assert (a.parent_tree, a.batches, a.rounds, a.child, a.variants) == ("/x", [2], 3, True, "unmasked")


def test_rounds_alternate_the_trees_and_the_report_is_their_medians():
    a = T.parse(["--parent-tree", "/parent", "--batches", "1", "--rounds", "2"])
    calls = []
    mine_out = [canned([5.0, 5.2], [5.1, 5.3], [5.4, 5.6], 20.0), canned([5.1, 5.1], [5.2, 5.2], [5.5, 5.5], 22.0)]
    parent_out = [{"steps_ms": {"1": {"unmasked": [5.0, 5.0]}}, "blend_pair_us": {}}, {"steps_ms": {"1": {"unmasked": [5.2, 5.4]}}, "blend_pair_us": {}}]

    def spawn(args, root, variants):
        calls.append((root, tuple(variants)))
        return (parent_out if root == "/parent" else mine_out)[sum(1 for r, _ in calls if r == root) - 1]
    mine, parent, pair = T.measure(a, spawn)
    assert calls == [("/parent", ("unmasked",)), (ROOT, ("unmasked", "masked", "masked_dd"))] * 2, "parent, this tree, parent, this tree"
    assert mine["1"]["unmasked"] == [5.0, 5.2, 5.1, 5.1] and parent["1"] == [5.0, 5.0, 5.2, 5.4] and pair == {"1": [20.0, 22.0]}
    row = T.report(a, mine, parent, pair)["batches"]["1"]
    assert row["unmasked"] == {"median_ms": 5.1, "min_ms": 5.0, "max_ms": 5.2, "runs": 4}
    assert row["masked"]["median_ms"] == pytest.approx(5.2) and row["masked_dd"]["median_ms"] == pytest.approx(5.5)
    assert row["masked_minus_unmasked_ms"] == pytest.approx(0.1) and row["masked_minus_unmasked_percent"] == pytest.approx(100 * 0.1 / 5.1)
    assert row["masked_dd_minus_unmasked_ms"] == pytest.approx(0.4) and row["blend_pair_us"] == 21.0
    assert row["parent_unmasked"]["median_ms"] == pytest.approx(5.1) and row["unmasked_minus_parent_unmasked_ms"] == pytest.approx(0.0)
    # without a parent tree: no parent rows, and only this tree is spawned
    calls.clear()
    b = T.parse(["--batches", "1", "--rounds", "1"])
    row = T.report(b, *T.measure(b, lambda args, root, variants: (calls.append(root), mine_out[0])[1]))["batches"]["1"]
    assert calls == [ROOT] and "parent_unmasked" not in row


def test_summary():
    assert T.summary([3.0, 1.0, 2.0]) == {"median_ms": 2.0, "min_ms": 1.0, "max_ms": 3.0, "runs": 3}
