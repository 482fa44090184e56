"""Hole filling on the device: a push-pull pyramid on the cyclic panorama.

    filler = HoleFiller(B, 3, H, W, device)
    mid, hole = interp.from_bidirectional(r, prev, frame, 0.5)        # FrameInterpolator(fill="none")
    dense, empty = filler.fill(mid, hole)                              # three launches at 512x1024, capturable

    dense, empty = fill_holes(src, hole)                               # one shot

What is known is averaged into a pyramid of 2 x 2 blocks (pull), the pyramid is expanded back bilinearly (push) and a level takes
the coarser one only where it knows nothing itself: a valid pixel keeps its bits, a hole takes the nearest scale at which something
is known.  The left and right edges of the panorama are neighbours (the push wraps its columns), the poles are not (rows are
clamped).  ``weight`` is a soft validity in [0, 1]: a pixel of weight 0.25 ends a quarter of the way from the filled value to its
own.  A value that is not finite counts as a hole.  The filling is gather-only: the same bits on every run.  ``FrameInterpolator(fill=
"pushpull")`` and ``Reprojector(fill=True)`` / ``DepthPropagator(fill=True)`` call it for their own holes.  There is no CPU path:
tensors on the host are refused (PfError).
"""
from __future__ import annotations

import contextlib
from typing import Optional

import torch

from . import _lib
from ._lib import PfError


def _library(device, lib):
    """The product's library for a cuda/ROCm device; `lib` (a handle of the tests' host emulation) lifts the device rule."""
    if lib is not None:
        return lib
    if torch.device(device).type != "cuda":
        raise PfError("hole filling needs tensors on a cuda/ROCm device; there is no CPU fallback")
    return _lib.load()


def _fit(t, shape, what: str, device, dtype=torch.float32):
    """A contiguous tensor of exactly this dtype, shape and device: nothing is converted or copied behind the caller's back."""
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_contiguous() or tuple(t.shape) != tuple(shape) \
            or t.device != device:
        got = f"{t.dtype} {tuple(t.shape)} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise PfError(f"{what} must be a contiguous {dtype} tensor {tuple(shape)} on {device}, got {got}")
    return t


def _meet(a: torch.Tensor, b: torch.Tensor) -> bool:
    pa, pb = a.data_ptr(), b.data_ptr()
    return pa < pb + b.numel() * b.element_size() and pb < pa + a.numel() * a.element_size()


class HoleFiller:
    """The holes of B maps [C,H,W] (C = 1..4) closed from a push-pull pyramid, with the pyramid allocated here: ``fill`` launches
    three times on the current stream for maps up to about 600 000 pixels (two more launches per level beyond),
    allocates nothing, never synchronises and can be captured into a HIP graph.  ``fill_levels`` runs the same arithmetic one
    level per launch (2 L + 2 launches): it is the yardstick of the tests and of profiles/time_fill.py and gives the same bits."""

    def __init__(self, B: int, C: int, H: int, W: int, device, lib=None):
        self.lib = _library(device, lib)
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if min(B, H, W) < 1 or not 1 <= C <= 4:
            raise PfError(f"HoleFiller: B, C, H, W = {B}, {C}, {H}, {W} (C = 1..4)")
        self.B, self.C, self.H, self.W = B, C, H, W
        self.L = self.lib.fill_levels(H, W)
        nbytes = self.lib.fill_bytes(B, C, H, W)                    # refuses the geometry the library does not take
        dev = self.device
        self.scratch = torch.zeros(nbytes // 4, dtype=torch.float32, device=dev)
        self.out = torch.zeros(B, C, H, W, dtype=torch.float32, device=dev)
        self.empty = torch.zeros(B, dtype=torch.uint8, device=dev)
        # the pyramid inside scratch (csrc/pf_fill.h): w0, then the values and the weights of the levels 1..L
        self.dims = [(H, W)]
        for _ in range(self.L):
            h, w = self.dims[-1]
            self.dims.append((max(1, (h + 1) // 2), max(1, (w + 1) // 2)))
        self.w0 = self.scratch[:B * H * W].view(B, H, W)
        self.levels, o = [], B * H * W
        for h, w in self.dims[1:]:
            v = self.scratch[o:o + B * C * h * w].view(B, C, h, w)
            o += B * C * h * w
            self.levels.append((v, self.scratch[o:o + B * h * w].view(B, h, w)))
            o += B * h * w
        assert o * 4 == nbytes, (o * 4, nbytes)

    def _args(self, what, src, hole, weight, out):
        B, C, H, W, dev = self.B, self.C, self.H, self.W, self.device
        _fit(src, (B, C, H, W), f"{what}: src", dev)
        _fit(hole, (B, H, W), f"{what}: hole", dev, torch.uint8)
        if weight is not None:
            _fit(weight, (B, H, W), f"{what}: weight", dev)
        out = self.out if out is None else _fit(out, (B, C, H, W), f"{what}: out", dev)
        if out is not src and out.data_ptr() != src.data_ptr() and _meet(out, src):
            raise PfError(f"{what}: out overlaps src without being src")
        for name, t in (("hole", hole), ("weight", weight)):
            if t is not None and _meet(out, t):
                raise PfError(f"{what}: out overlaps {name}")
        for name, t in (("src", src), ("hole", hole), ("weight", weight), ("out", out)):
            if t is not None and (_meet(self.scratch, t) or _meet(self.empty, t)):
                raise PfError(f"{what}: {name} overlaps the filler's own buffers")
        return out

    def _on(self):
        return torch.cuda.device(self.device) if self.device.type == "cuda" else contextlib.nullcontext()

    def fill(self, src, hole, weight: Optional[torch.Tensor] = None, out=None):
        """(out fp32 [B,C,H,W], empty uint8 [B]).  src fp32 [B,C,H,W]; hole uint8 [B,H,W], non-zero: missing; weight fp32 [B,H,W]
        or None.  out: where to write (default ``self.out``); it may be src itself (in place), nothing else of the inputs.
        empty[b] = 1 where image b has no valid pixel at all; its out is 0."""
        out = self._args("HoleFiller.fill", src, hole, weight, out)
        with self._on():
            self.lib.fill_pushpull(src, hole, weight, out, self.empty, self.scratch)
        return out, self.empty

    def fill_levels(self, src, hole, weight: Optional[torch.Tensor] = None, out=None):
        """``fill`` through the level-by-level entry points: prepare, L pulls, the apex step, L pushes.  The same bits; afterwards
        ``self.w0`` and ``self.levels`` hold the pyramid (the values filled)."""
        out = self._args("HoleFiller.fill_levels", src, hole, weight, out)
        lib = self.lib
        with self._on():
            lib.fill_prepare(src, hole, weight, self.w0)
            maps = [(src, self.w0)] + self.levels
            for (fv, fw), (cv, cw) in zip(maps[:-1], maps[1:]):
                lib.fill_pull_level(fv, fw, cv, cw)
            tv, tw = maps[-1]
            lib.fill_push_level(None, tv, tw, out if self.L == 0 else tv, self.empty)
            for l in range(self.L - 1, -1, -1):
                fv, fw = maps[l]
                lib.fill_push_level(maps[l + 1][0], fv, fw, out if l == 0 else fv)
        return out, self.empty


def fill_holes(src: torch.Tensor, hole: torch.Tensor, weight: Optional[torch.Tensor] = None, lib=None):
    """(out [B,C,H,W], empty uint8 [B]) of one map with its holes closed; the pyramid is allocated per call (for a video use
    ``HoleFiller``)."""
    if not isinstance(src, torch.Tensor) or src.dim() != 4:
        raise PfError("fill_holes: src must be a tensor [B,C,H,W]")
    B, C, H, W = src.shape
    with torch.no_grad():
        f = HoleFiller(B, C, H, W, src.device, lib=lib)
        return f.fill(src, hole, weight)
