"""The lifecycle the four resident models share on the host (`MI355XUNet`, `MI355XVAE`, `MI355XUpscaler`, `MI355XTAESD`): a C handle
created under the device guard, its parameters loaded from a checkpoint or a generator, a workspace that grows when a call exceeds it,
the counters of the last run, and the launch table of a profiled one.  The library exports these alike for every family, as
`ld_<family>_<op>` (csrc/runtime.h `Model`); what a family computes stays in its own wrapper.
"""
from __future__ import annotations

import ctypes as C
from typing import Callable, Dict, Iterator, Tuple, Union

import torch

from ._lib import F16, F32, check, lib

WeightSource = Union[Dict[str, torch.Tensor], Callable[[str, tuple], torch.Tensor]]


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


class ResidentModel:
    family = ""                  # "unet" | "vae" | "esrgan" | "taesd"
    key_prefixes = ("",)         # checkpoint-key prefixes tried, in order, for every parameter of a state dict
    reserve_rank = 3             # arguments of ld_<family>_reserve: (batch, h, w); the UNet adds the context tokens

    def _fn(self, op: str):
        return getattr(lib(), f"ld_{self.family}_{op}")

    def _create(self, weights: WeightSource, *config) -> None:
        """The handle (`config`: what ld_<family>_create takes in front of it) with every parameter loaded; no workspace yet."""
        self._h = C.c_void_p()
        self._reserved = (0,) * self.reserve_rank
        self.reserve_epoch = 0   # bumped whenever the workspace moves: a captured hipGraph of an older epoch is stale
        with torch.cuda.device(self.device):
            check(self._fn("create")(*config, C.byref(self._h)), f"ld_{self.family}_create")
            for key, shape in self._params():
                self._load_param(key, shape, weights)
        torch.cuda.synchronize(self.device)

    def _params(self) -> Iterator[Tuple[str, tuple]]:
        """(name, shape as the checkpoint stores it) of every parameter, in the library's order."""
        name, ndim, shape = C.c_char_p(), C.c_int(), (C.c_int64 * 4)()
        for i in range(self._fn("param_count")(self._h)):
            check(self._fn("param_info")(self._h, i, C.byref(name), C.byref(ndim), shape), "param_info")
            yield name.value.decode(), tuple(int(shape[k]) for k in range(ndim.value))

    def param_shapes(self) -> Dict[str, tuple]:
        """{parameter name (checkpoint key minus the family's prefix): shape as the checkpoint stores it}"""
        if getattr(self, "_param_shapes", None) is None:
            self._param_shapes = dict(self._params())
        return dict(self._param_shapes)

    def _load_param(self, key: str, shp: tuple, src: WeightSource) -> None:
        if callable(src):
            t = src(key, shp)
        else:
            t = next((src[p + key] for p in self.key_prefixes if p + key in src), None)
            if t is None:
                raise KeyError(f"checkpoint is missing '{key}'")
        if tuple(t.shape) != shp:
            raise ValueError(f"'{key}': expected shape {shp}, got {tuple(t.shape)}")
        if t.dtype not in (torch.float16, torch.float32):
            t = t.float()
        t = t.to(self.device).contiguous()
        check(self._fn("load_param")(self._h, key.encode(), t.data_ptr(), F32 if t.dtype == torch.float32 else F16, _stream()), f"load_param({key})")

    # -- workspace
    def _grown(self, *shape) -> tuple:
        """The shape a call of `shape` leaves reserved: the larger of it and the reserved one, per axis."""
        return tuple(max(s, m) for s, m in zip(shape, self._reserved))

    def _ensure(self, *shape) -> None:
        """Lazy re-reserve (the reference accepts any batch and size): grow the workspace when a call exceeds it instead of failing
        with ERR_SHAPE."""
        if self._grown(*shape) != self._reserved:
            self._reserve(*self._grown(*shape))

    def _reserve(self, *shape) -> None:
        """(Re)size the workspace.  It frees and reallocates: `_reserved` is written once the library has the new one."""
        with torch.cuda.device(self.device):
            check(self._fn("reserve")(self._h, *shape), f"ld_{self.family}_reserve")
        self._reserved = tuple(shape)
        self.reserve_epoch += 1
        self._workspace_moved()

    def _workspace_moved(self) -> None:
        """What else dies with the old workspace (the UNet: its context and captured graphs)."""

    def __del__(self):
        try:
            if getattr(self, "_h", None) and self._h.value:
                self._fn("destroy")(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass

    @property
    def workspace_bytes(self) -> int:
        return self._fn("workspace_bytes")(self._h)

    def plan_bytes(self, b: int, h: int, w: int) -> int:
        """The workspace a (b, h, w) call needs: a host-only dry run of the executor (the UNet exports none)."""
        return self._fn("plan_bytes")(self._h, b, h, w)

    # -- the last run
    @property
    def last_launches(self) -> int:
        return self._fn("last_launches")(self._h)

    @property
    def last_flops(self) -> float:
        return self._fn("last_flops")(self._h)

    def profile_launches(self) -> list:
        """Per launch of the last profiled run: [(what, (a, b, c, d), flops, microseconds, kernel)] in launch order."""
        buf = C.create_string_buffer(1 << 18)
        check(self._fn("profile_launches")(self._h, buf, len(buf)), "profile_launches")
        out = []
        for line in buf.value.decode().splitlines():
            what, a, b, c, d, fl, us, kern = line.split("\t")
            out.append((what, (int(a), int(b), int(c), int(d)), float(fl), float(us), kern))
        return out
