"""Peaked attention inputs for the lazy softmax rescale of attention.hip (helper module of tests/test_errbound_cpu.py and
tests/test_routes_gpu.py; plain torch, built on the CPU so that a case has the same bits wherever it runs).

flash_attn2_kernel and flash_attn512_kernel keep a softmax reference m_ref per query that starts at the maximum of the first 32-key subtile
and moves only when a later subtile's maximum exceeds it by more than TAU (exp2 domain); a move rescales O and l, shifts the scores and
rewrites the MFMA's C operand.  randn inputs at scale 1 never move it after the first subtile.  make() starts from randn at scale 1 and plants
key rows k[b, j, head] = a q[b, r, head], a chosen so that the planted score stands a stated jump (exp2 units) above query r's reference at
that point of the recursion:

  spike    two rows of every three get one key in a later subtile; the keys walk through every position 0..31 of a subtile and every later
           subtile, the last valid key of a ragged Lk included; jumps cycle through 6 (below TAU: no move, P rises to 2^6), 10, 20, 40.
           Every third row stays flat: some lanes of a wave move, others take delta = 0.
  stairs   chosen rows get one key in EVERY later subtile, each 10 above the reference the previous one left: the reference moves in every
           subtile, the rescales compound, both LDS buffers see a move.
  descend  the dominant keys (25 / 40 above every other key of the row) sit in the first subtile: everything later is an fp16 subnormal
           or zero in P, no late move.
  offset   channel 0 of every head: k += 6, q = +-q0 alternating by row, q0 ~ 4 sqrt(d) (_offset_q0): every score of a row shifts by about +-35
           exp2 units (times 1 + k0 / 6 with k's own randn k0: a spread of 5.8 units that peaks the shifted rows as well).  The first reference is
           large (about +47 / -23: the shift plus the largest of 32 such spreads), the scores cancel against it in the accumulator.  The
           reference is a running maximum: it moves only where a subtile brings a new record by more than TAU, which a shift common to all keys
           cannot arrange in every subtile for either sign — the odd rows are the even rows with the order of their keys reversed, and a few
           per cent up to a third of either kind move late (make() asserts the first references, not a share of moves).  A larger shift widens
           the spread and ds with it (at +-100: 17 units, ds 0.05, an element bound of 10 % of |o|) without exercising anything else.
  onehot   a few rows get one key more than 40 units above every other key of the row, in the first, middle and last subtiles and on both
           sides of the tile boundaries: every other weight is below 2^-25 of it and rounds to 0 in fp16, l is exactly 1 on both denominator
           paths and the output row must equal that key's v row bit for bit.

A planted key is one key for EVERY query of its (batch, head): query r' sees it at a (q_r' . q_r) / |q_r|^2 of its planted score, a random
score of standard deviation (planted score) / sqrt(d).  The builder therefore plants subtile by subtile against the reference the fp64
recursion holds at that point, reads every fact from an fp64 run of the recursion over the finished inputs, and asserts
  * every planted row reaches its stated jump (at most one planted key in 64 may fall short and is then left out of the facts);
  * every threshold comparison of every row clears TAU by more than twice that row's score error bound (the ds of errbound.attention_ref):
    the kernel's sequence of moves is decided by the inputs, not by rounding.  A row that lands inside that window has its query scaled by
    1.03 until it is outside (offset: its channels 1.. rotated by one; it is an input like any other; at most one query in RESCALED_CAP of a case, 5.5 % at most over ATTN_PEAKED;
    facts["rescaled"] names them);
  * every onehot margin is >= 40.
With `causal` keys are planted at j <= r only, the diagonal key j = r of late rows included (it shares its subtile with -inf entries).
"""
import functools
import math
import os
import re

import torch

import errbound as EB

LOG2E = 1.4426950408889634
SUB = 32                                   # keys per softmax step of both kernels
PATTERNS = ("spike", "stairs", "descend", "offset", "onehot")
SPIKE_JUMPS = (6.0, 10.0, 20.0, 40.0)
STAIR_JUMP = 10.0
DESCEND_JUMPS = (25.0, 40.0)
ONEHOT_JUMP = 64.0
ONEHOT_MARGIN = 40.0                       # fp16 rounds a weight below 2^-25 to zero: 15 units to spare
RESCALED_CAP = 8                           # at most one query in 8 of a case may need scaling out of the rounding window
ROOM = 0.5                                 # planted above the stated jump by this much: the fp16 rounding of a q is 2^-11 of the score


def _tau():
    """TAU of attention.hip (both kernels declare the same constant)."""
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "lightdiffusion_amd", "csrc", "attention.hip")).read()
    vals = re.findall(r"constexpr float TAU = ([0-9.]+)f;", src)
    assert len(vals) == 2 and len(set(vals)) == 1, vals
    return float(vals[0])


TAU = _tau()


def _offset_q0(d):
    """The fp16 number nearest 4 sqrt(d) (within an eighth of it) whose product with the kernels' fp32 scale * log2(e), rounded to fp32 and then
    to fp16 as the kernels do, lies closest to the exact q0 log2(e) / sqrt(d): every row of `offset` holds this one value, so its rounding error
    would be one error shared by all rows (4 sqrt(d) itself: 5.7708 -> 5.7695, every 35-unit shift scaled by 1 - 2.2e-4, a signed bias of -2e-4
    that is the input's doing); the value chosen here is off by less than 2^-19."""
    c2 = torch.tensor(1.0 / math.sqrt(d), dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
    bits = torch.arange(0x3C00, 0x7C00, dtype=torch.int16)                       # the fp16 numbers in [1, inf)
    cand = bits.view(torch.float16)
    cand = cand[((cand.double() - 4.0 * math.sqrt(d)).abs() <= 0.5 * math.sqrt(d))]
    exact = cand.double() * (LOG2E / math.sqrt(d))
    err = ((cand.float() * c2).half().double() - exact).abs() / exact
    best = int(err.argmin())
    assert float(err[best]) < 2.0 ** -19, float(err[best])
    return float(cand[best])


def _heads(t, heads):
    """[b][L][heads d] -> the view [b][heads][L][d] (writes go through)."""
    b, l, c = t.shape
    return t.view(b, l, heads, c // heads).transpose(1, 2)


def scores(q, k, heads, causal):
    """fp64 scores of the fp16 inputs in the exp2 domain, [b][heads][Lq][Lk] (-inf above the diagonal), and the bound ds of what the kernel's
    fp16-rounded q * scale * log2(e) and its fp32 accumulation can move each of them by (errbound.attention_ref's ds, in exp2 units)."""
    qd, kd = _heads(q, heads).double(), _heads(k, heads).double()
    c2 = LOG2E / math.sqrt(qd.shape[-1])
    s = (qd @ kd.transpose(-1, -2)) * c2
    ds = EB.U * c2 * (qd.abs() @ kd.abs().transpose(-1, -2)) + 2.0 ** -22 * s.abs()
    if causal:
        mask = torch.ones(s.shape[-2], s.shape[-1], dtype=torch.bool).triu(1)
        s.masked_fill_(mask, float("-inf"))
        ds.masked_fill_(mask, 0.0)
    return s, ds


def recursion(s):
    """The kernels' lazy reference in fp64 over scores s [..][Lk]: per 32-key subtile t the maximum minus the reference before it (gap; t = 0:
    the maximum itself, which the reference takes whatever it is) and whether the reference moves there (move; t >= 1: gap > TAU)."""
    lk = s.shape[-1]
    nsub = (lk + SUB - 1) // SUB
    pad = torch.full(s.shape[:-1] + (nsub * SUB - lk,), float("-inf"), dtype=s.dtype)
    mx = torch.cat([s, pad], -1).view(s.shape[:-1] + (nsub, SUB)).amax(-1)
    m = mx[..., 0].clone()
    gaps, moves = [m.clone()], [torch.zeros_like(m, dtype=torch.bool)]
    for t in range(1, nsub):
        g = mx[..., t] - m
        mv = g > TAU
        m = torch.where(mv, mx[..., t], m)
        gaps.append(g)
        moves.append(mv)
    return torch.stack(gaps, -1), torch.stack(moves, -1)


def _stride(n):
    return next(p for p in (37, 41, 43, 47, 53) if n % p)


def _rows_for(cand, specials, g, take):
    """`take` rows of the candidate list for (batch, head) number g: each g starts where the one before stopped; g = 0 starts with the specials."""
    if g == 0:
        cand = [r for r in specials if r in cand] + [r for r in cand if r not in specials]
        return cand[:take]
    o = (g * take) % len(cand)
    return (cand[o:] + cand[:o])[:take]


def _plan(pattern, g, lq, lk, causal):
    """[(row, key, jump)] of one (batch, head): distinct keys, keys <= row when causal."""
    nsub = (lk + SUB - 1) // SUB
    last = lq - 1
    specials = [0, SUB - 1, last]
    out = []
    if pattern == "spike":
        if causal:
            rows = [r for r in range(SUB, lq) if r % 3 == 0 or (r % 3 == 1 and r >= SUB + 2) or r == last]
            out = [(r, r if (r % 3 == 0 or (r == last and r % 3 == 2)) else r - 2) for r in rows]
        else:
            nslots = lk - SUB
            st = _stride(nslots)
            rows = _rows_for([r for r in range(lq) if r % 3 != 2 or r == last], specials, g, nslots)
            out = [(r, lk - 1 - (n * st) % nslots) for n, r in enumerate(rows)]
        return [(r, j, SPIKE_JUMPS[(n + n // 4) % 4]) for n, (r, j) in enumerate(out)]
    if pattern == "stairs":
        if causal:
            # every third row first (those get a key in every subtile they see), then the rows between them take what is left
            cand = [r for r in range(SUB + 2, lq) if r % 3 == 1 or r == last]
            rows = cand[::(len(cand) + SUB - 1) // SUB]
            rows = rows if last in rows else rows[:-1] + [last]
            rows = rows + [r for r in range(SUB + 2, lq) if r % 3 == 0 and r not in rows]
        else:
            rows = _rows_for([r for r in range(lq) if r % 3 == 0 or r in specials], specials, g, SUB)
        used = set()
        for n, r in enumerate(rows):
            for t in range(1, nsub):
                if causal and t > r // SUB:
                    break
                if causal and t == r // SUB:
                    free = [r]                                                   # the diagonal key
                else:
                    free = [SUB * t + (n + 11 * t + i) % SUB for i in range(SUB)]
                j = next((j for j in free if j < lk and j not in used), None)
                if j is not None and (causal or n < SUB):
                    used.add(j)
                    out.append((r, j, STAIR_JUMP))
        return out
    if pattern == "descend":
        rows = _rows_for([r for r in range(lq) if r % 3 != 2 or r == last], specials, g, SUB)
        used = set()
        for n, r in enumerate(rows):
            j = (5 * n) % SUB
            j = r if (causal and j > r) else j
            if j < lk and j not in used:
                used.add(j)
                out.append((r, j, DESCEND_JUMPS[n % 2]))
        return out
    raise ValueError(pattern)


def _onehot_keys(lk):
    nsub = (lk + SUB - 1) // SUB
    mid = SUB * (nsub // 2)
    keys = [0, SUB - 1, SUB, 2 * SUB - 1, 2 * SUB, mid + 17, SUB * (nsub - 1), lk - 1, 4 * SUB - 1, 4 * SUB]
    return sorted({j for j in keys if 0 <= j < lk})


def _plant_onehot(qh, kh, causal):
    """Per (batch, head) one row per key of _onehot_keys: rows 0, 31, Lq - 1 first, then spread over the queries; a row is taken only if its
    query is nearly orthogonal (|cos| < 0.4) to those already taken, so that one row's key stays small for the others.  Four sweeps set each
    key ONEHOT_JUMP above the row's largest other score (a later key changes the earlier rows' other scores a little)."""
    b, h, lq, d = qh.shape
    lk = kh.shape[2]
    c2 = LOG2E / math.sqrt(d)
    keys = _onehot_keys(lk)
    nominal = [0, SUB - 1, lq - 1] + [(n * (lq - 1)) // len(keys) for n in range(1, len(keys))]
    qd = qh.double()
    qn = qd / qd.norm(dim=-1, keepdim=True)
    pairs = []
    for bi in range(b):
        for hi in range(h):
            taken = []
            for n, j in enumerate(keys):
                start = max(nominal[n], j) if causal else nominal[n]
                order = list(range(start, lq)) + ([] if causal else list(range(0, start)))
                for r in order:
                    if all(r != r2 and abs(float(qn[bi, hi, r] @ qn[bi, hi, r2])) < 0.4 for r2, _ in taken):
                        taken.append((r, j))
                        break
            pairs += [(bi, hi, r, j) for r, j in taken]
    idx = torch.tensor(pairs, dtype=torch.long)
    bi, hi, ri, ji = idx.unbind(1)
    qsel = qd[bi, hi, ri]                                                        # [n][d]
    own = (qsel * qsel).sum(-1) * c2
    kd = kh.double().contiguous()
    col = torch.arange(lk)
    hidden = (col.unsqueeze(0) == ji.unsqueeze(1)) | ((col.unsqueeze(0) > ri.unsqueeze(1)) if causal else False)
    for _ in range(4):
        for n in range(len(pairs)):
            other = ((kd[bi[n], hi[n]] @ qsel[n]) * c2).masked_fill(hidden[n], float("-inf"))
            target = max(float(other.max()), 0.0) + ONEHOT_JUMP + ROOM
            kd[bi[n], hi[n], ji[n]] = (qsel[n] * (target / float(own[n]))).half().double()
    kh[bi, hi, ji] = kd[bi, hi, ji].half()
    return idx


def _plant(pattern, qh, kh, causal):
    """Plant spike / stairs / descend subtile by subtile: the keys of subtile t are set against the reference that the recursion over the
    finished subtiles 0..t-1 holds (descend, t = 0: against the row's largest background score).  Returns [(b, h, row, key, t)], jumps."""
    b, h, lq, d = qh.shape
    lk = kh.shape[2]
    c2 = LOG2E / math.sqrt(d)
    nsub = (lk + SUB - 1) // SUB
    plan = [(bi, hi, r, j, jump) for bi in range(b) for hi in range(h) for (r, j, jump) in _plan(pattern, bi * h + hi, lq, lk, causal)]
    idx = torch.tensor([p[:4] for p in plan], dtype=torch.long)
    jumps = torch.tensor([p[4] for p in plan], dtype=torch.float64)
    qd = qh.double()
    qsq = (qd * qd).sum(-1) * c2                                                 # [b][h][lq]: the score of a key equal to the query
    if pattern == "descend":
        base = ((qd @ kh.double().transpose(-1, -2)) * c2)
        if causal:
            base.masked_fill_(torch.ones(lq, lk, dtype=torch.bool).triu(1), float("-inf"))
        m = base.amax(-1)
    else:
        m = None
    rows = torch.arange(lq).view(1, 1, lq, 1)
    for t in range(nsub):
        sel = (idx[:, 3] // SUB) == t
        if bool(sel.any()):
            bi, hi, ri, ji = idx[sel].unbind(1)
            a = (m[bi, hi, ri] + jumps[sel] + ROOM) / qsq[bi, hi, ri]
            assert bool((a > 0).all())
            kh[bi, hi, ji] = (qd[bi, hi, ri] * a.unsqueeze(-1)).half()
        if pattern == "descend":
            break
        keys = torch.arange(t * SUB, min(lk, (t + 1) * SUB))
        s = (qd @ kh[:, :, keys].double().transpose(-1, -2)) * c2
        if causal:
            s.masked_fill_(keys.view(1, 1, 1, -1) > rows, float("-inf"))
        mx = s.amax(-1)
        m = mx if t == 0 else torch.where(mx - m > TAU, mx, m)
    return torch.cat([idx, (idx[:, 3:4] // SUB)], 1), jumps


@functools.lru_cache(maxsize=None)
def make(pattern, b, heads, lq, lk, d, causal=False, seed=0):
    """(q, k, v, facts): fp16 CPU tensors [b][L][heads d] (shared between callers: do not write to them) and
    facts = {moves [b][heads][Lq][nsub] bool: where the fp64 recursion moves the reference after the first subtile; gaps: the compared
    differences; planted [n][5] (b, head, row, key, subtile) with jumps [n]; onehot [n][4] (b, head, row, key); rescaled [b][heads][Lq] bool: the
    queries that were scaled out of the rounding window (at most one in RESCALED_CAP)}."""
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(b, n, heads * d, generator=g).half() for n in (lq, lk, lk))
    qh, kh = _heads(q, heads), _heads(k, heads)
    planted, jumps, onehot = torch.zeros(0, 5, dtype=torch.long), torch.zeros(0, dtype=torch.float64), torch.zeros(0, 4, dtype=torch.long)
    if pattern == "offset":
        kh[..., 0] += 6.0
        sign = 1.0 - 2.0 * (torch.arange(lq) % 2).half()
        qh[..., 0] = _offset_q0(d) * sign
    elif pattern == "onehot":
        onehot = _plant_onehot(qh, kh, causal)
    else:
        planted, jumps = _plant(pattern, qh, kh, causal)
    # rows with a threshold comparison inside the rounding window: scale the query until it is outside
    rescaled = torch.zeros(b, heads, lq, dtype=torch.bool)
    for _ in range(40):
        s, ds = scores(q, k, heads, causal)
        gaps, moves = recursion(s)
        window = 2.0 * ds.amax(-1, keepdim=True)
        close = (((gaps - TAU).abs() <= window) & torch.isfinite(gaps))[..., 1:].any(-1)
        if not bool(close.any()):
            break
        rescaled |= close
        if pattern == "offset":                                # (channel 0 keeps its exactly scaled value: the other channels rotate by one)
            qh[..., 1:][close] = qh[..., 1:][close].roll(1, -1)
        else:
            qh[close] = (qh[close].float() * 1.03).half()
    assert not bool(close.any()), f"{pattern}: {int(close.sum())} rows keep a threshold comparison within the scores' rounding error"
    assert int(rescaled.sum()) * RESCALED_CAP <= rescaled.numel(), f"{pattern}: {int(rescaled.sum())} of {rescaled.numel()} queries rescaled"
    bi, hi, ri, ji = (planted[:, c] for c in range(4))
    if pattern in ("spike", "stairs"):
        # (a query scaled out of the rounding window may have turned an earlier near-move into a move: that plant then stands on a higher
        # reference than it was set against, and the row is left out of the facts)
        ok = gaps[bi, hi, ri, planted[:, 4]] >= jumps
        assert int((~ok).sum()) * 64 <= len(planted), f"{pattern}: {int((~ok).sum())} of {len(planted)} planted keys short of their jump"
        planted, jumps = planted[ok], jumps[ok]
    elif pattern == "descend":
        later = s[..., SUB:].amax(-1) if lk > SUB else torch.full(s.shape[:-1], float("-inf"), dtype=s.dtype)
        assert bool((s[bi, hi, ri, ji] - later[bi, hi, ri] >= jumps).all())
    if pattern == "offset":
        first = gaps[..., 0]
        assert float(first[..., 0::2].median()) >= 30.0 and float(first[..., 1::2].median()) <= -15.0, "offset: first references"
    if len(onehot):
        bo, ho, ro, jo = onehot.unbind(1)
        own = s[bo, ho, ro, jo]
        rest = s[bo, ho, ro].clone()
        rest[torch.arange(len(onehot)), jo] = float("-inf")
        margin = own - rest.amax(-1)
        assert bool((margin >= ONEHOT_MARGIN).all()), f"onehot margins down to {float(margin.min()):.1f}"
    facts = {"moves": moves, "gaps": gaps, "planted": planted, "jumps": jumps, "onehot": onehot, "rescaled": rescaled}
    return q, k, v, facts


def onehot_rows_equal_v(o, v, heads, facts):
    """True when every onehot row of the output o [b][Lq][heads d] equals its key's v row bit for bit (a [n] mask per pair otherwise)."""
    d = o.shape[-1] // heads
    oh = facts["onehot"].to(o.device)
    if len(oh) == 0:
        return True
    bo, ho, ro, jo = oh.unbind(1)
    got = o.view(o.shape[0], o.shape[1], heads, d)[bo, ro, ho]
    want = v.to(o.device).view(v.shape[0], v.shape[1], heads, d)[bo, jo, ho]
    same = (got.view(torch.int16) == want.view(torch.int16)).all(-1)
    return True if bool(same.all()) else same
