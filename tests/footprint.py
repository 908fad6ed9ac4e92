"""The guard harness of the footprint tests (helper module): WHERE a kernel reads and writes, not what it computes.

Every value test of the suite hands a kernel exact-size torch tensors: what lies behind an operand is finite left-overs of earlier tensors, what
lies behind an output is allocator slack, an output that a kernel skips can still hold the right value from the previous identical call, and the
scratch holds whatever the last operator left.  A kernel that over-reads a tail and zeroes only one side of the product (0 x finite = 0), that stores
a row or eight columns too many, that skips an element or that reads scratch it never wrote passes all of them.

place() copies an operand into the middle of a larger flat buffer of its own and returns a view with the requested row pitch and batch stride:

    [ front guard 64 KiB | batch 0: rows x pitch | inter-batch gap | batch 1 ... | back guard max(64 KiB, 512 rows x pitch bytes) ]

The front guard, the back guard, the pitch gap behind every row (columns cols .. pitch-1) and the gap between two batch elements hold one bit
pattern, the poison.  512 rows is the height of the tallest tile of the contraction kernels (the 128x512 halo tile): one whole stray tile row of
stores still lands in the guard, not in a neighbour's memory.  Guard sizes are multiples of 256 bytes, so an operand keeps the alignment the
executors' arenas give it.

Poisons.  Inputs: fp16 NaN 0x7E00 (fp32 operands: 0x7FC00000) in one run, +Inf 0x7C00 (0x7F800000) in another — Inf for a leak through a max or a
compare that drops NaN.  Outputs: guards and gaps 0xAAAA (the sentinel of tests/test_end_convs_gpu.py), the interior NaN before the call.  Scratch:
guards of 0xAA bytes in front of ws and behind ws + ws_bytes, the interior bytes 0xFF in one run (NaN as fp16 and as fp32, -1 as a counter) and
0x00 in the other.

hold() runs one call three times — plain, on exact-size operands as the value tests do; NaN guards with 0xFF scratch; Inf guards with 0x00
scratch — and reports, per guarded run: a route other than the plain one, the first output element whose BITS differ from the plain run, the
first output element still NaN (never written), the first touched guard or gap element of every operand, the first touched scratch-guard byte.
No tolerance: the kernels are deterministic (no float atomics), so a call whose footprint is right is bit-identical to the plain call that
tests/test_routes_gpu.py holds to fp64.

Poison only what the header does not make the caller's duty (include/ld_mi355x.h): the key padding Lk .. round8(Lk) of a transposed V stays
zero and is part of the operand handed to place(); rows and columns the header calls "read as zeros" or "not read" are poison.
"""
from __future__ import annotations

from collections import namedtuple

import torch

FRONT_BYTES = 64 << 10          # in front of every operand and of the scratch
BACK_BYTES = 64 << 10           # behind it, at least
TALLEST_TILE = 512              # rows of the 128x512 halo tile: the back guard holds that many rows of the operand's pitch

NAN16, INF16, SENTINEL16 = 0x7E00, 0x7C00, 0xAAAA
NAN32, INF32, SENTINEL32 = 0x7FC00000, 0x7F800000, 0xAAAAAAAA
SCRATCH_GUARD = 0xAA
POISONS = {"nan": (NAN16, NAN32), "inf": (INF16, INF32), "sentinel": (SENTINEL16, SENTINEL32)}
RUNS = (("nan", 0xFF), ("inf", 0x00))          # (input poison, scratch interior byte) of the two guarded runs

_INT = {torch.float16: torch.int16, torch.float32: torch.int32, torch.int32: torch.int32, torch.int16: torch.int16}

# region: 'front' / 'back' (row, col count from the operand's first element in units of its pitch: row -1 is the row in front, row == rows the
# first row behind; for a batched operand relative to the last batch element), 'gap' (col >= cols: the pitch gap of that row; row >= rows: the
# gap between two batch elements), 'interior' (an element of the operand itself)
Touch = namedtuple("Touch", "operand region batch row col")


def _signed(bits: int, itemsize: int) -> int:
    width = 8 * itemsize
    return bits - (1 << width) if bits >= 1 << (width - 1) else bits


def _bits(poison, dtype) -> int:
    if isinstance(poison, str):
        p16, p32 = POISONS[poison]
        return p16 if dtype in (torch.float16, torch.int16) else p32
    return int(poison)


def _round256(nbytes: int) -> int:
    return (nbytes + 255) // 256 * 256


class Placed:
    """One operand inside its guarded buffer.  `view`: the operand as the call sees it ([batch][rows][cols] strided, or the shape it was given
    where that is contiguous); `flat`: the whole buffer as integers."""

    def __init__(self, name, shape, dtype, device, poison, rows_behind=TALLEST_TILE, pitch=None, batch_stride=None):
        shape = tuple(shape)
        self.name, self.shape, self.dtype = name, shape, dtype
        if len(shape) == 3:
            self.batch, self.rows, self.cols = shape
        else:
            self.batch, self.cols = 1, shape[-1]
            self.rows = 1
            for s in shape[:-1]:
                self.rows *= s
        item = torch.empty(0, dtype=dtype).element_size()
        self.pitch = self.cols if pitch is None else int(pitch)
        self.bs = self.rows * self.pitch if batch_stride is None else int(batch_stride)
        assert self.pitch >= self.cols and self.bs >= self.rows * self.pitch, "pitch / batch stride smaller than the operand"
        self.front = FRONT_BYTES // item
        self.body = self.batch * self.bs
        self.back = _round256(max(BACK_BYTES, rows_behind * self.pitch * item)) // item
        self.poison = _signed(_bits(poison, dtype), item)
        self.flat = torch.full((self.front + self.body + self.back,), self.poison, dtype=_INT[dtype], device=device)
        geom = ((self.batch, self.rows, self.cols), (self.bs, self.pitch, 1), self.front)
        self.iview = self.flat.as_strided(*geom)
        self.guard = torch.ones(self.flat.shape, dtype=torch.bool, device=device)
        self.guard.as_strided(*geom).fill_(False)
        v = self.flat.view(dtype).as_strided(*geom)
        if len(shape) != 3:
            v = v[0]
            if self.pitch == self.cols:
                v = v.view(shape)
        self.view = v

    def locate(self, i: int) -> Touch:
        rel = i - self.front
        if rel < 0:
            return Touch(self.name, "front", 0, rel // self.pitch, rel % self.pitch)
        if rel >= self.body:
            rel -= (self.batch - 1) * self.bs
            return Touch(self.name, "back", self.batch - 1, rel // self.pitch, rel % self.pitch)
        b, o = divmod(rel, self.bs)
        r, c = divmod(o, self.pitch)
        return Touch(self.name, "gap" if (c >= self.cols or r >= self.rows) else "interior", b, r, c)


def place(t: torch.Tensor, poison, rows_behind: int = TALLEST_TILE, pitch=None, batch_stride=None, name: str = "x") -> Placed:
    """Copy t ([batch][rows][cols] when 3-D, else rows x t.shape[-1]) into the middle of a larger flat buffer; guards, pitch gaps and inter-batch
    gaps hold `poison` ('nan', 'inf', 'sentinel' or a bit pattern of t's width)."""
    p = Placed(name, t.shape, t.dtype, t.device, poison, rows_behind, pitch, batch_stride)
    p.view.copy_(t)
    return p


def place_output(shape, dtype, device, rows_behind: int = TALLEST_TILE, pitch=None, batch_stride=None, name: str = "y") -> Placed:
    """An output: guards and gaps the sentinel, every interior element NaN until the call writes it."""
    p = Placed(name, shape, dtype, device, "sentinel", rows_behind, pitch, batch_stride)
    p.iview.fill_(_signed(_bits("nan", dtype), p.flat.element_size()))
    return p


def _first(mask: torch.Tensor):
    """Index (a tuple) of the first True element of mask, None when there is none."""
    if not bool(mask.any()):
        return None
    flat = mask.reshape(-1).to(torch.uint8)
    i = int(torch.argmax(flat))
    idx = []
    for s in reversed(mask.shape):
        i, r = divmod(i, s)
        idx.append(r)
    return tuple(reversed(idx))


def check_guards(p: Placed):
    """The first guard, pitch-gap or inter-batch-gap element of p that no longer holds the poison, as a Touch; None when all do."""
    i = _first((p.flat != p.poison) & p.guard)
    return None if i is None else p.locate(i[0])


def check_written(p: Placed, upto=None):
    """The first element of the output p that is still NaN (never written, or NaN came in through a leak), as a Touch; None when every element
    was written.  upto: only the first `upto` elements of a flat output are expected (the rest must still be NaN: the second Touch)."""
    nan = _signed(_bits("nan", p.dtype), p.flat.element_size())
    still = p.iview == nan
    if upto is not None:
        flat = still.reshape(-1)
        i, j = _first(~flat[upto:]), _first(flat[:upto])
        if i is not None:
            return Touch(p.name, "unasked", 0, 0, upto + i[0])
        return None if j is None else Touch(p.name, "interior", 0, 0, j[0])
    i = _first(still)
    return None if i is None else Touch(p.name, "interior", *i)


def first_difference(p: Placed, plain: torch.Tensor, upto=None):
    """The first element of p whose bits differ from the plain run's output, as a Touch."""
    a = p.iview
    b = plain.contiguous().view(_INT[plain.dtype]).reshape(a.shape if upto is None else (1, 1, -1))
    if upto is not None:
        a, b = a.reshape(1, 1, -1)[..., :upto], b[..., :upto]
    i = _first(a != b)
    return None if i is None else Touch(p.name, "interior", *i)


class Scratch:
    """A scratch buffer with guards of its own: [64 KiB of 0xAA | ws_bytes | 64 KiB of 0xAA].  One allocation, grown on demand, armed per run."""

    def __init__(self, device):
        self.device, self.buf, self.n = device, None, 0

    def arm(self, nbytes: int, fill: int) -> torch.Tensor:
        total = FRONT_BYTES + _round256(nbytes) + BACK_BYTES
        if self.buf is None or self.buf.numel() < total:
            self.buf = None
            self.buf = torch.empty(total, dtype=torch.uint8, device=self.device)
        self.n = nbytes
        self.buf[:FRONT_BYTES] = SCRATCH_GUARD
        self.buf[FRONT_BYTES:FRONT_BYTES + nbytes] = fill
        self.buf[FRONT_BYTES + nbytes:FRONT_BYTES + nbytes + BACK_BYTES] = SCRATCH_GUARD
        return self.buf[FRONT_BYTES:FRONT_BYTES + nbytes]

    def check(self):
        i = _first(self.buf[:FRONT_BYTES] != SCRATCH_GUARD)
        if i is not None:
            return Touch("ws", "front", 0, 0, i[0] - FRONT_BYTES)
        i = _first(self.buf[FRONT_BYTES + self.n:FRONT_BYTES + self.n + BACK_BYTES] != SCRATCH_GUARD)
        return None if i is None else Touch("ws", "back", 0, 0, self.n + i[0])


def _spec(v):
    return (v, {}) if isinstance(v, torch.Tensor) else (v[0], dict(v[1]))


def probe(call, inputs: dict, outputs: dict, ws_bytes: int = 0, scratch: Scratch = None, plain_scratch=None, sync=None, runs=RUNS):
    """Run `call` plain and under each guarded run; return (plain route, plain outputs, findings).

    call(I, O, ws) -> route: I / O map operand names to tensors (exact-size contiguous ones in the plain run, strided views into guarded buffers
    otherwise: the call passes data_ptr() and the strides), ws is a uint8 tensor of exactly ws_bytes (None when ws_bytes == 0).
    inputs:  name -> tensor, or (tensor, dict(pitch=, batch_stride=, poison=)).  A tensor of another dtype than fp16 / fp32 / int32 is not placed.
    outputs: name -> (shape, dtype), or (shape, dtype, dict(pitch=, batch_stride=, rows_behind=, upto=callable(route) -> the leading elements of a
             flat output that must be written, all others must stay untouched)).
    findings: [(run, kind, Touch or text)], kind in 'route', 'differs', 'unwritten', 'guard'."""
    ins = {k: _spec(v) for k, v in inputs.items()}
    outs = {k: (v[0], v[1], dict(v[2]) if len(v) > 2 else {}) for k, v in outputs.items()}
    dev = next(iter(ins.values()))[0].device
    sync = sync or (torch.cuda.synchronize if dev.type == "cuda" else (lambda: None))
    plain_scratch = plain_scratch or (lambda n: torch.zeros(n, dtype=torch.uint8, device=dev))
    scratch = scratch or Scratch(dev)

    pI = {k: t.contiguous() for k, (t, _) in ins.items()}
    pO = {k: torch.empty(shape, dtype=dt, device=dev) for k, (shape, dt, _) in outs.items()}
    route = call(pI, pO, plain_scratch(ws_bytes) if ws_bytes else None)
    sync()

    findings = []
    for poison, fill in runs:
        gI = {}
        for k, (t, kw) in ins.items():
            kw = dict(kw)
            gI[k] = place(t, kw.pop("poison", poison), name=k, **kw)
        gO = {k: place_output(shape, dt, dev, kw.get("rows_behind", TALLEST_TILE), kw.get("pitch"), kw.get("batch_stride"), name=k)
              for k, (shape, dt, kw) in outs.items()}
        ws = scratch.arm(ws_bytes, fill) if ws_bytes else None
        got = call({k: p.view for k, p in gI.items()}, {k: p.view for k, p in gO.items()}, ws)
        sync()
        run = f"{poison}/0x{fill:02X}"
        if got != route:
            findings.append((run, "route", f"{got!r} instead of {route!r}"))
        for k, p in gO.items():
            upto = outs[k][2].get("upto")
            upto = None if upto is None else upto(got)
            for kind, t in (("guard", check_guards(p)), ("unwritten", check_written(p, upto)), ("differs", first_difference(p, pO[k], upto))):
                if t is not None:
                    findings.append((run, kind, t))
        for p in gI.values():
            t = check_guards(p)
            if t is not None:
                findings.append((run, "guard", t))
        if ws is not None:
            t = scratch.check()
            if t is not None:
                findings.append((run, "guard", t))
        del gI, gO
    return route, pO, findings


def hold(call, inputs, outputs, ws_bytes=0, expect=None, what="", **kw):
    """probe(), then: the pinned route (expect: a string, or a predicate of the route), and no finding."""
    route, plain, findings = probe(call, inputs, outputs, ws_bytes, **kw)
    if expect is not None:
        assert expect(route) if callable(expect) else route == expect, f"{what}: route {route!r}"
    assert not findings, f"{what} [{route}]: " + "; ".join(f"{run} {kind} {t}" for run, kind, t in findings)
    return route, plain
