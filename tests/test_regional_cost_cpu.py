"""CPU: tools/regional_cost.py rehearsed without a device — its arguments, the alternation of the trees over the rounds, and the figures it derives
from canned child output (medians, the differences between the cases, the cost per extra group, the two acceptance flags against the parent's
spread, the kernel pair).  The measurement itself needs the GPU; the child refuses to run without one."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import regional_cost as T      # noqa: E402


def canned(plain, multi_off, one_group, three_groups, pair):
    """what this tree's two processes of a round print: (a) + (b), then (b) + (c) + (d) with (b) 0.05 ms slower there"""
    return ({"steps_ms": {"1": {"plain": list(plain), "multi_off": list(multi_off)}}, "kernel_pair_us": {"1": pair - 1.0}},
            {"steps_ms": {"1": {"multi_off": [x + 0.05 for x in multi_off], "one_group": list(one_group), "three_groups": list(three_groups)}},
             "kernel_pair_us": {"1": pair}})


def test_arguments():
    a = T.parse([])
    assert (a.steps, a.repeats, a.rounds, a.batches, a.parent_tree, a.child) == (20, 4, 2, [1, 8], None, False)
    assert a.out == os.path.join(ROOT, "profiles", "regional_cost.json") and a.package_root == ROOT and a.variants == "plain,multi_off,one_group,three_groups"
    a = T.parse(["--parent-tree", "/x", "--batches", "2", "--rounds", "3", "--child", "--variants", "plain"])
    assert (a.parent_tree, a.batches, a.rounds, a.child, a.variants) == ("/x", [2], 3, True, "plain")


def test_rounds_alternate_the_trees_and_the_report_is_their_medians():
    a = T.parse(["--parent-tree", "/parent", "--batches", "1", "--rounds", "2"])
    calls = []
    mine_out = [canned([5.0, 5.2], [7.0, 7.2], [6.9, 7.1], [9.0, 9.2], 20.0), canned([5.1, 5.1], [7.1, 7.1], [7.0, 7.0], [9.1, 9.1], 22.0)]
    parent_out = [{"steps_ms": {"1": {"plain": [5.0, 5.0], "multi_off": [7.0, 7.1]}}, "kernel_pair_us": {}},
                  {"steps_ms": {"1": {"plain": [5.2, 5.4], "multi_off": [7.2, 7.3]}}, "kernel_pair_us": {}}]

    def spawn(args, root, variants):
        calls.append((root, tuple(variants)))
        n = sum(1 for r, _ in calls if r == root) - 1
        return parent_out[n] if root == "/parent" else mine_out[n // 2][n % 2]
    mine, parent, pair = T.measure(a, spawn)
    assert calls == [("/parent", ("plain", "multi_off")), (ROOT, ("plain", "multi_off")), (ROOT, ("multi_off", "one_group", "three_groups"))] * 2, \
        "per round: the parent, this tree on the parent's sequence, this tree's new cases"
    assert mine["1"]["plain"] == [5.0, 5.2, 5.1, 5.1] and parent["1"]["multi_off"] == [7.0, 7.1, 7.2, 7.3]
    assert pair == {"1": [20.0, 22.0]} and mine["1"]["multi_off"] == [7.0, 7.2, 7.1, 7.1]
    assert mine["1"]["multi_off_beside_new"] == pytest.approx([7.05, 7.25, 7.15, 7.15])
    row = T.report(a, mine, parent, pair)["batches"]["1"]
    assert row["plain"] == {"median_ms": 5.1, "min_ms": 5.0, "max_ms": 5.2, "runs": 4}
    assert row["one_group"]["median_ms"] == pytest.approx(7.0) and row["three_groups"]["median_ms"] == pytest.approx(9.1)
    assert row["one_group_minus_multi_off_ms"] == pytest.approx(-0.15) and row["three_groups_minus_one_group_ms"] == pytest.approx(2.1)
    assert row["extra_group_ms"] == pytest.approx(1.05) and row["kernel_pair_us"] == 21.0
    assert row["parent_plain"]["median_ms"] == pytest.approx(5.1) and row["plain_minus_parent_plain_ms"] == pytest.approx(0.0)
    assert row["parent_multi_off"]["median_ms"] == pytest.approx(7.15) and row["one_group_minus_parent_multi_off_ms"] == pytest.approx(-0.15)
    assert row["plain_within_parent_spread"] is True and row["one_group_not_slower_than_parent_multi_off_by_more_than_its_spread"] is True
    # the flags fall where the figures leave the parent's spread
    slow = {"1": dict(mine["1"], plain=[5.5] * 4, one_group=[7.7] * 4)}
    row = T.report(a, slow, parent, pair)["batches"]["1"]
    assert row["plain_within_parent_spread"] is False and row["one_group_not_slower_than_parent_multi_off_by_more_than_its_spread"] is False
    # without a parent tree: no parent rows, and only this tree is spawned
    calls.clear()
    b = T.parse(["--batches", "1", "--rounds", "1"])
    row = T.report(b, *T.measure(b, lambda args, root, variants: (calls.append(root), mine_out[0][len(calls) - 1])[1]))["batches"]["1"]
    assert calls == [ROOT, ROOT] and "parent_plain" not in row and "plain_within_parent_spread" not in row


def test_summary():
    assert T.summary([3.0, 1.0, 2.0]) == {"median_ms": 2.0, "min_ms": 1.0, "max_ms": 3.0, "runs": 3}
