"""CPU: the guard harness holds itself, and the footprint module leaves no pinned route out.

Self-test of tests/footprint.py on a torch stand-in "kernel" (y = x w^T through an fp32 slab in the scratch) with one seeded defect at a time: a
store in front of the output, one behind it, eight columns into a pitch gap, a skipped interior element, an input tail read from the guard and
multiplied by zero, a scratch word read before it was written, a store behind the scratch.  Each is reported at its operand, region and index;
the clean stand-in is clean under both poisons.  In the plain run a stray access that leaves the exact-size tensor goes nowhere — the
allocator slack nobody looks at — which is why the value tests cannot see these defects.

Ledger: every instantiation name of test_routes_gpu.route_names() is visited by a parametrization of tests/test_footprint_gpu.py, every
row of every route table is one of its cases, and no case carries a skip or an expected failure.
"""
import inspect

import pytest
import torch

import footprint as FP
from footprint import Touch

M, N, K = 6, 16, 24


def _reach(t, offset):
    """The element `offset` elements from t's first one in t's storage (a 1-element view), None when the storage ends before it."""
    at = t.storage_offset() + offset
    room = t.untyped_storage().nbytes() // t.element_size()
    return t.as_strided((1,), (1,), at) if 0 <= at < room else None


def standin(defect=None):
    def call(I, O, ws):
        x, w, y = I["x"], I["w"], O["y"]
        acc = x.float() @ w.float().t()
        slab = ws.view(torch.float32)[:M * N].view(M, N)
        if defect == "scratch":                       # an accumulator the kernel takes for zero: word 7 is read before anything wrote it
            acc = acc + slab.reshape(-1)[7] * 0.0
        slab.copy_(acc)
        acc = slab.clone()
        if defect == "leak":                          # the k-step runs 8 past K on the last row and zeroes only the weight's side
            tail = _reach(x, (M - 1) * x.stride(0) + K)
            if tail is not None:
                acc[M - 1] += tail.float() * 0.0
        out = acc.half()
        if defect == "skip":
            keep = y[3, 5].clone()
            y.copy_(out)
            y[3, 5] = keep
        else:
            y.copy_(out)
        stray = {"before": [-1], "behind": [(M - 1) * y.stride(0) + N], "gap8": [2 * y.stride(0) + N + j for j in range(8)] if y.stride(0) > N else []}
        for off in stray.get(defect, []):
            e = _reach(y, off)
            if e is not None:
                e.fill_(1.0)
        if defect == "ws_behind":
            e = _reach(ws, ws.numel())
            if e is not None:
                e.fill_(1)
        return "standin"
    return call


def operands(pitch=None):
    g = torch.Generator().manual_seed(5)
    x, w = torch.randn(M, K, generator=g).half(), torch.randn(N, K, generator=g).half()
    out = ((M, N), torch.float16, dict(pitch=pitch)) if pitch else ((M, N), torch.float16)
    return {"x": x, "w": w}, {"y": out}


def run(defect, pitch=None):
    ins, outs = operands(pitch)
    return FP.probe(standin(defect), ins, outs, 4 * M * N + 64)[2]


@pytest.mark.parametrize("pitch", [None, N + 8])
def test_clean_standin_is_clean_under_both_poisons(pitch):
    ins, outs = operands(pitch)
    route, plain, findings = FP.probe(standin(), ins, outs, 4 * M * N + 64)
    assert route == "standin" and findings == []
    assert torch.equal(plain["y"], (ins["x"].float() @ ins["w"].float().t()).half())
    FP.hold(standin(), ins, outs, 4 * M * N + 64, expect="standin")


BOTH = [f"{poison}/0x{fill:02X}" for poison, fill in FP.RUNS]
DEFECTS = [
    ("before", None, "guard", Touch("y", "front", 0, -1, N - 1), BOTH),
    ("behind", None, "guard", Touch("y", "back", 0, M, 0), BOTH),
    ("gap8", N + 8, "guard", Touch("y", "gap", 0, 2, N), BOTH),
    ("skip", None, "unwritten", Touch("y", "interior", 0, 3, 5), BOTH),
    ("leak", None, "differs", Touch("y", "interior", 0, M - 1, 0), BOTH),           # NaN x 0 and Inf x 0 are both NaN
    ("scratch", None, "differs", Touch("y", "interior", 0, 0, 0), ["nan/0xFF"]),    # 0x00 bytes are the zeros the kernel took for granted
    ("ws_behind", None, "guard", Touch("ws", "back", 0, 0, 4 * M * N + 64), BOTH),
]


@pytest.mark.parametrize("defect,pitch,kind,touch,runs", DEFECTS, ids=[d[0] for d in DEFECTS])
def test_seeded_defect_is_located(defect, pitch, kind, touch, runs):
    findings = run(defect, pitch)
    for r in BOTH:
        got = [(k, t) for rr, k, t in findings if rr == r]
        if r in runs:
            assert (kind, touch) in got, (r, got)
            assert all(t.operand == touch.operand for k, t in got if k != "route"), got     # and at no other operand
        else:
            assert got == [], (r, got)
    with pytest.raises(AssertionError, match=touch.region):
        ins, outs = operands(pitch)
        FP.hold(standin(defect), ins, outs, 4 * M * N + 64)


def test_place_geometry_and_poisons():
    """Guard sizes (64 KiB in front; behind max(64 KiB, 512 rows of the pitch), multiples of 256 bytes), the bit patterns, and a touched element
    of every region of a batched, pitched operand named by batch, row and column."""
    t = torch.arange(2 * 3 * 8, dtype=torch.float16).view(2, 3, 8)
    p = FP.place(t, "nan", pitch=16, batch_stride=4 * 16, name="q")
    assert p.front * 2 == 64 << 10 and p.back * 2 == max(64 << 10, 512 * 16 * 2) and (p.back * 2) % 256 == 0
    assert torch.equal(p.view, t) and p.view.stride() == (64, 16, 1)
    assert int(p.flat[0]) == 0x7E00 and int(p.flat[p.front + 8]) == 0x7E00 and int(p.flat[-1]) == 0x7E00
    assert FP.check_guards(p) is None
    wide = FP.place(torch.zeros(4, 4096, dtype=torch.float16), "inf")
    assert wide.back * 2 == 512 * 4096 * 2 and int(wide.flat[0]) == 0x7C00
    f = FP.place(torch.zeros(5, dtype=torch.float32), "nan")
    assert f.front * 4 == 64 << 10 and int(f.flat[0]) == 0x7FC00000 and f.view.shape == (5,)
    o = FP.place_output((2, 3, 8), torch.float16, "cpu", pitch=16, batch_stride=64)
    assert int(o.flat[0]) == 0xAAAA - 0x10000 and bool(torch.isnan(o.view).all())
    assert FP.check_written(o) == Touch("y", "interior", 0, 0, 0)
    o.view.fill_(1.0)
    assert FP.check_written(o) is None and FP.check_guards(o) is None
    for off, want in [(p.front - 16 - 3, Touch("y", "front", 0, -2, 13)), (p.front + 16 + 8, Touch("y", "gap", 0, 1, 8)),
                      (p.front + 3 * 16 + 2, Touch("y", "gap", 0, 3, 2)), (p.front + 64 + 2 * 16 + 15, Touch("y", "gap", 1, 2, 15)),
                      (p.front + 128 + 16 + 1, Touch("y", "back", 1, 5, 1))]:
        keep = o.flat[off].clone()
        o.flat[off] = 0
        assert FP.check_guards(o) == want, (off, FP.check_guards(o))
        o.flat[off] = keep
    o.view[1, 2, 7] = float("nan")
    assert FP.check_written(o) == Touch("y", "interior", 1, 2, 7)


def test_scratch_guards_and_fill():
    s = FP.Scratch("cpu")
    ws = s.arm(1000, 0xFF)
    assert ws.numel() == 1000 and bool((ws == 0xFF).all()) and s.check() is None
    assert bool(torch.isnan(ws[:996].view(torch.float32)).all()) and bool(torch.isnan(ws.view(torch.float16)).all()) and int(ws[:4].view(torch.int32)) == -1
    s.buf[FP.FRONT_BYTES - 1] = 0
    assert s.check() == Touch("ws", "front", 0, 0, -1)
    ws = s.arm(300, 0x00)                      # re-armed smaller: the guard moves up to the new end
    assert bool((ws == 0).all()) and s.check() is None
    s.buf[FP.FRONT_BYTES + 300] = 0
    assert s.check() == Touch("ws", "back", 0, 0, 300)


def test_partial_secondary_output():
    """A flat output of which only a leading part is asked for: the rest must stay untouched, the part must be written."""
    o = FP.place_output((100,), torch.float32, "cpu", rows_behind=0)
    assert o.back * 4 == 64 << 10
    o.view[:64] = 1.0
    assert FP.check_written(o, upto=64) is None
    assert FP.check_written(o, upto=70) == Touch("y", "interior", 0, 0, 64)
    assert FP.check_written(o, upto=60) == Touch("y", "unasked", 0, 0, 60)


# ------------------------------------------------------------------ the ledger

def _cases():
    """{test name: (argnames, argvalues)} of every parametrization of tests/test_footprint_gpu.py that names a route, and every mark in the module."""
    import test_footprint_gpu as G
    cases, marks = {}, list(G.pytestmark) if isinstance(G.pytestmark, (list, tuple)) else [G.pytestmark]
    for name, fn in inspect.getmembers(G, inspect.isfunction):
        if not name.startswith("test_") or fn.__module__ != G.__name__:
            continue
        for m in getattr(fn, "pytestmark", []):
            marks.append(m)
            if m.name == "parametrize":
                names = [a.strip() for a in m.args[0].split(",")]
                for v in m.args[1]:
                    marks += list(getattr(v, "marks", []))
                if "route" in names:
                    cases[name] = (names, list(m.args[1]))
    return cases, marks


def test_every_pinned_route_has_a_footprint_case():
    import test_footprint_gpu as G
    import test_routes_gpu as R
    cases, marks = _cases()
    assert not [m.name for m in marks if m.name in ("skip", "skipif", "xfail")], "a footprint case is skipped or expected to fail"
    tables = {"test_attention_footprint": R.ATTN_ROUTES, "test_attention_qkv_seam_footprint": G.QKV_SEAM, "test_linear_footprint": R.LINEAR_ROUTES,
              "test_linear_ln_footprint": R.LN_ROUTES, "test_conv_footprint": R.CONV_ROUTES, "test_conv_vae_out_footprint": G.VAE_OUT,
              "test_groupnorm_conv_footprint": R.GN_CONV_ROUTES, "test_conv_gn_partials_footprint": R.GN_PART_ROUTES, "test_conv_skip_footprint": R.SKIP_ROUTES}
    assert set(cases) == set(tables)
    rows = left_out = 0
    visited = set()
    for test, table in tables.items():
        names, values = cases[test]
        assert len(table) > 0
        rows += len(table)
        left_out += sum(1 for row in table if tuple(row) not in {tuple(v) for v in values})
        for v in values:
            for part in v[names.index("route")].split(";"):
                visited.add(part)
                visited.update(part.split("+"))
        print(f"{test}: {len(values)} cases of {len(table)} rows")
    assert len(G.QKV_SEAM) == sum(1 for row in R.ATTN_PEAKED if row[0] == "qkv") > 0 and len(G.VAE_OUT) == 1
    assert left_out / rows == 0.0, f"{left_out} of {rows} route rows have no footprint case"
    missing = sorted(R.route_names() - visited)
    assert not missing, f"pinned by tests/test_routes_gpu.py, no footprint case: {missing}"
