"""What every executor-against-operator-chain test shares (helper module; its CPU control: tests/test_chain_harness_cpu.py).

The chain side: `ChainBase`, the weight plumbing and the tap list of tests/unet_chain.py, vae_chain.py, esrgan_chain.py and taesd_chain.py, and
`Feat`.  The test side, used by tests/test_{unet,vae,esrgan,taesd,adverse}_chain_gpu.py (and, for the record, test_clip_chain_gpu.py):

  B1  `same_launches`   the chain's launch list against the executor's profile table, entry by entry;
  B2  `differs`, `bits_held`, `same_bits`   torch.equal with the shape history A, B, A; no tolerance;
  B3  `held`, `partials_held`, `every_stage`, `stages_held`   EB.check per tap, the worst figures per stage kind; `tap_images`: a tap cut to
      a fixed subset of its images (a full-width case evaluates its fp64 references on two images, one at a time);
  `record`, `stage_record`   the one LD_WRITE_PARITY=1 writer into profiles/; `side_fixture`   the module-scoped cache of a module's Side.

pytest rewrites no assertion of a helper module: every assert here carries its message.
"""
from __future__ import annotations

import json
import os

import pytest
import torch

import errbound as EB
from lightdiffusion_amd import weights as W

PROFILES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles")


# ------------------------------------------------------------------ the chain side

class Feat:
    """An activation [n][H][W][C] and, where its producer wrote them, the GroupNorm partial statistics of it."""

    def __init__(self, t, part=None):
        self.t, self.part = t, part


class ChainBase:
    """Weights: the checkpoint's fp32 masters -> fp16, in the layouts the kernels read, by the seam's own operators; and the taps.
    shapes: name -> shape; prefix: what the synthetic checkpoint's keys carry in front of the names; source: a WeightSource
    (name, shape -> fp32 master), None: the synthetic checkpoint of `seed`."""

    def __init__(self, shapes: dict, device="cuda:0", seed: int = 0, source=None, prefix: str = ""):
        from lightdiffusion_amd import ops
        self.ops, self.dev, self.seed, self.source = ops, torch.device(device), seed, source
        self.shapes, self.prefix = shapes, prefix
        self._w = {}
        self.taps = []

    def master(self, name):
        if self.source is not None:
            return self.source(self.prefix + name, self.shapes[name])
        return W.synth_tensor(self.prefix + name, self.shapes[name], self.seed)

    def _cached(self, key, make):
        if key not in self._w:
            self._w[key] = make()
        return self._w[key]

    def vec(self, name):
        return self._cached(name, lambda: self.master(name).half().to(self.dev).contiguous())

    def mat(self, name):
        """[O][I] (a Linear, or a 1x1 convolution's [O][I][1][1])."""
        return self._cached(name, lambda: self.master(name).half().reshape(self.shapes[name][0], -1).to(self.dev).contiguous())

    def oihw(self, name):
        """fp16 [O][I][k][k], the checkpoint's layout (what the fp64 references take)."""
        return self._cached(("oihw", name), lambda: self.master(name).half().to(self.dev).contiguous())

    def conv3(self, name):
        """[O][9 I] tap-major from the fp32 master, as a load repacks it."""
        return self._cached(("c3", name), lambda: self.ops.repack_conv_weight(self.master(name).to(self.dev)))

    def tap(self, kind, name, inp, par, out, **more):
        self.taps.append(dict(kind=kind, name=name, inp=inp, par=par, out=out, kernel=self.ops.last_kernel(), launches=self.ops.last_launches(), **more))
        return out


# ------------------------------------------------------------------ B1

def same_launches(name, taps, table):
    """The chain's launches, [(layer, kernel)], equal to the executor's launch table entry by entry; every tap launched something."""
    mine = [(t["name"], k) for t in taps for k in t["launches"].split(";") if k]
    for i, ((layer, a), b) in enumerate(zip(mine, table)):
        assert a == b, f"{name}: launch {i} differs at {layer}: the chain ran {a}, the executor {b}"
    assert len(mine) == len(table), (f"{name}: the chain has {len(mine)} launches, the executor {len(table)}; first unmatched: "
                                     f"{mine[len(table)] if len(mine) > len(table) else table[len(mine)]}")
    assert all(t["launches"] for t in taps), f"{name}: taps without a launch: {[t['name'] for t in taps if not t['launches']]}"
    return mine


# ------------------------------------------------------------------ B2

def differs(a, b):
    d = (a != b)
    idx = d.nonzero()[0].tolist()
    return f"{int(d.sum())} of {d.numel()} elements differ, first at {idx}: executor {float(a[tuple(idx)])!r}, chain {float(b[tuple(idx)])!r}"


def bits_held(got, want, what):
    """torch.equal(executor, chain) of one tensor or of a tuple of them."""
    gs, ws = (got, want) if isinstance(want, tuple) else ((got,), (want,))
    assert len(gs) == len(ws), f"{what}: {len(gs)} results, the chain has {len(ws)}"
    for k, (g, w) in enumerate(zip(gs, ws)):
        part = what if len(ws) == 1 else f"{what}, result {k}"
        assert g.shape == w.shape, f"{part}: shape {tuple(g.shape)}, the chain's {tuple(w.shape)}"
        assert torch.equal(g, w), f"{part}: {differs(g, w)}"


def same_bits(name, want, run, others=()):
    """run(name) is `want` bit for bit, also with every other case run in between on the same handle (shape history A, B, A)."""
    bits_held(run(name), want, name)
    for other in others:
        run(other)
        bits_held(run(name), want, f"{name} after {other}")


# ------------------------------------------------------------------ B3

def held(y, ref, bound, what, bias_extra=0.0, keep=None, **where):
    """EB.check; the bias statistic of fewer than 10^4 elements gets its chance level EB.rtn_noise on top of BIAS_TOL."""
    extra = EB.rtn_noise(EB.independent_roundings(ref, keep)) if ref.numel() < 10 ** 4 else 0.0
    return EB.check(y, ref, bound, what, bias_extra=bias_extra + extra, keep=keep, **where)


def partials_held(part, y, what):
    """A producer's GroupNorm partials against fp64 sums of the STORED fp16 outputs (tests/test_routes_gpu.py::test_conv_gn_partials_route);
    any chunking of an image's pixels: the VAE's are one chunk per tile."""
    n, cout = y.shape[0], y.shape[-1]
    yg = y.double().reshape(n, -1, 32, cout // 32)
    hw = yg.shape[1]
    got = part.double().sum(1)
    want = torch.stack([yg.sum((1, 3)), (yg * yg).sum((1, 3))], -1)
    tol = torch.stack([yg.abs().sum((1, 3)), (yg * yg).sum((1, 3))], -1) * (EB.c_acc(hw * cout // 32) + 2.0 ** -22) + EB.TINY
    assert bool(((got - want).abs() <= tol).all()), f"{what}: partial statistics, error / tolerance {float(((got - want).abs() / tol).max()):.3g}"


def stage_record(worst: dict, tol: float = 1.0) -> dict:
    """{stage kind: [worst error / bound, largest signed bias]} as the parity record; tol: the unit of the signed bias."""
    return {k: {"worst_error_over_bound": round(v[0], 4), "signed_bias_over_tolerance": round(v[1] / tol, 4)} for k, v in sorted(worst.items())}


EVERY_IMAGE = "every image"     # as the `images` of every_stage: all images of a tap, one at a time


def image_indices(images, n):
    """The image subset of a case table (negative: counted from the end; EVERY_IMAGE: all) as sorted indices into a tap of n images."""
    if images == EVERY_IMAGE:
        return list(range(n))
    assert all(-n <= i < n for i in images), f"image subset {tuple(images)} of a tap of {n} images"
    return sorted({i % n for i in images})


def tap_images(tap, images):
    """The tap restricted to `images` of the tap['n'] images it ran on: every tensor of its inputs, output(s) and partial statistics cut to
    those images — [n][...] by index, the rows [n L][C] of a linear as L rows per image.  Parameters (tap['par']) are shared by the images.
    Only for stages that are separable per image (a convolution, GroupNorm's statistics, attention, the rows of a linear)."""
    n = tap["n"]
    idx = image_indices(images, n)

    def cut(t):
        if isinstance(t, (tuple, list)):
            return type(t)(cut(e) for e in t)
        if not isinstance(t, torch.Tensor):
            return t
        at = torch.as_tensor(idx, device=t.device)
        if t.shape[0] == n:
            return t.index_select(0, at)
        assert t.dim() == 2 and t.shape[0] % n == 0, f"{tap['name']}: a tensor of shape {tuple(t.shape)} in a tap of {n} images"
        return t.reshape(n, t.shape[0] // n, t.shape[1]).index_select(0, at).reshape(-1, t.shape[1])

    cutd = dict(tap, n=len(idx), inp={k: cut(v) for k, v in tap["inp"].items()}, out=cut(tap["out"]))
    if tap.get("part") is not None:
        cutd["part"] = cut(tap["part"])
    return cutd


def every_stage(name, taps, stage_fn, images=None):
    """stage_fn(tap, what) -> [(error / bound, signed bias)] on every tap.  -> (the record per stage kind, the failed stages' messages).
    images: a fixed subset of images (negative: from the end).  A tap that carries its image count (tap['n']: a stage separable per image)
    is then evaluated on those images only, one image at a time (`tap_images`; the failure names the image) — the other images of such a
    tap are NOT looked at; a tap without 'n' is evaluated whole."""
    fails, worst = [], {}
    for tap in taps:
        what = f"{name} {tap['name']} [{tap.get('kernel') or tap['launches']}]"
        if images is None or "n" not in tap:
            views = [(tap, what)]
        else:
            views = ((tap_images(tap, [j]), f"{what} image {j}") for j in image_indices(images, tap["n"]))
        for view, where in views:
            try:
                for r, b in stage_fn(view, where):
                    w = worst.setdefault(tap["kind"], [0.0, 0.0])
                    w[0], w[1] = max(w[0], r), (b if abs(b) > abs(w[1]) else w[1])
            except AssertionError as e:
                fails.append(str(e))
    return stage_record(worst, EB.BIAS_TOL), fails


def stages_held(fails, taps):
    assert not fails, f"{len(fails)} of {len(taps)} stages outside their bound:\n" + "\n".join(fails[:12])


# ------------------------------------------------------------------ the record, the sides

def record(fname: str, case: str, what: dict) -> None:
    """With LD_WRITE_PARITY=1: merge `what` into the entry `case` of profiles/<fname> (a record, not an assertion)."""
    if os.environ.get("LD_WRITE_PARITY") != "1":
        return
    path = os.path.join(PROFILES, fname)
    have = json.load(open(path)) if os.path.exists(path) else {}
    have.setdefault(case, {}).update(what)
    with open(path, "w") as f:
        json.dump(have, f, indent=1, sort_keys=True)
        f.write("\n")


def side_fixture(make):
    """The module-scoped fixture `side`: side(*key) is make(*key), built once per key and dropped with the module."""
    @pytest.fixture(scope="module", name="side")
    def side():
        sides = {}

        def get(*key):
            if key not in sides:
                sides[key] = make(*key)
            return sides[key]
        yield get
        sides.clear()
        torch.cuda.empty_cache()
    return side
