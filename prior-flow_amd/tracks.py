"""Correspondence over more than one pair of a panoramic video: chained flows and point tracks.

    stream = FlowStream(model, iters=12, bidirectional=True, occlusion="sphere")
    chain = FlowChain(B, H, W, device)
    for frame in frames:
        r = stream(frame)
        if r is not None:
            chain.push(r)              # one launch behind the stream's step, capturable
    chain.forward, chain.visible       # flow(anchor -> last frame) on the anchor's grid [B,2,H,W]; the pixels still seen
    chain.backward                     # flow(last frame -> anchor) on the last frame's grid

    tracker = PointTracker(points, H, W)            # points [B,N,2] = (x, y) pixels
    pos, state = tracker.push(flow, occ)            # per pair; pos keeps the winding of x, tracker.pos_wrapped is x mod W

One statement does all of it (include/priorflow_hip.h: pf_flow_compose): p' = p + g^(p), g^ the model's cyclic sampler with the
seam un-wrapping of pf_fb_check, u never clipped to +-W/2, and one sticky state byte per point (TRK_OCCLUDED | TRK_POLE |
TRK_NONFINITE).  A point with a state other than 0 keeps being advanced; mask by ``state``.  There is no CPU path: tensors on
the host are refused (PfError).
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from ._lib import PfError
from .video import BidirectionalFlow

TRK_OCCLUDED, TRK_POLE, TRK_NONFINITE = _lib.PfLib.TRK_OCCLUDED, _lib.PfLib.TRK_POLE, _lib.PfLib.TRK_NONFINITE


def _library(device, lib):
    """The product's library for a cuda/ROCm device; `lib` (a handle of the tests' host emulation) lifts the device rule."""
    if lib is not None:
        return lib
    if torch.device(device).type != "cuda":
        raise PfError("flow chains and point tracks need tensors on a cuda/ROCm device; there is no CPU fallback")
    return _lib.load()


def _flow4(t, what):
    if not isinstance(t, torch.Tensor) or t.dim() != 4 or t.shape[1] != 2:
        raise PfError(f"{what}: expected a flow [B,2,H,W], got {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")


def compose_flow(f: torch.Tensor, g: torch.Tensor, state_f: Optional[torch.Tensor] = None, occ_g: Optional[torch.Tensor] = None,
                 out=None, lib=None):
    """(flow, state) of f followed by g: flow(x) = f(x) + g^(x + f(x)) on f's grid, [B,2,H,W]; state uint8 [B,H,W] = state_f |
    the new bits (occ_g: the mask that belongs to g, on g's grid; any non-zero byte counts).  out: the (flow, state) tensors to
    write into; the flow may be f itself.  One launch, capturable."""
    _flow4(f, "compose_flow: f")
    _flow4(g, "compose_flow: g")
    lib = _library(f.device, lib)
    if g.shape != f.shape or g.device != f.device:
        raise PfError(f"compose_flow: f {tuple(f.shape)} on {f.device} / g {tuple(g.shape)} on {g.device} do not fit")
    with torch.no_grad():
        f, g = f.float().contiguous(), g.float().contiguous()
        B, _, H, W = f.shape
        if out is None:
            out = (torch.empty_like(f), torch.empty(B, H, W, dtype=torch.uint8, device=f.device))
        flow, state = out
        lib.flow_compose([(f, state_f, g, occ_g, flow, state)])
    return flow, state


class FlowChain:
    """Flow from an anchor frame to the latest frame of B videos, and back, updated once per pair in one launch.

    ``push(r)`` takes what a bidirectional ``FlowStream`` returns for the pair (t-1, t), or a plain forward flow [B,2,H,W]:
      forward  <- compose(forward, r.forward, state, r.occ_forward)                    anchor -> t on the anchor's grid
      backward <- compose(r.backward, backward, r.occ_backward, backward_state)         t -> anchor on frame t's grid
    With a plain flow only ``forward`` moves (no occlusion bit) and ``backward`` is None until the next ``reset()``.
    Every buffer is allocated here; ``push`` reads nothing back and allocates nothing on the device, and runs on the current
    stream.  ``reset()`` re-anchors the chain at the first frame of the next pair pushed."""

    def __init__(self, B: int, H: int, W: int, device, lib=None):
        self._lib = _library(device, lib)
        if min(B, H, W) < 1:
            raise PfError(f"FlowChain: B, H, W = {B}, {H}, {W}")
        self.shape = (B, 2, H, W)
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=device)       # noqa: E731
        self._fw, self._fw_state = z(B, 2, H, W), z(B, H, W, dt=torch.uint8)
        # t -> anchor is written from the previous one (its g): a pair of buffers, `_cur` holds the latest
        self._bw = [z(B, 2, H, W), z(B, 2, H, W)]
        self._bw_state = [z(B, H, W, dt=torch.uint8), z(B, H, W, dt=torch.uint8)]
        self._cur = 0
        self._both = True
        self.length = 0

    def reset(self) -> None:
        """Forget the chain (zero flow, every pixel visible); the buffers stay."""
        for t in [self._fw, self._fw_state] + self._bw + self._bw_state:
            t.zero_()
        self._cur, self._both, self.length = 0, True, 0

    def push(self, r) -> "FlowChain":
        fw, st = self._fw, self._fw_state
        if isinstance(r, BidirectionalFlow):
            for t in (r.forward, r.backward):
                _flow4(t, "FlowChain.push")
                if tuple(t.shape) != self.shape:
                    raise PfError(f"FlowChain.push: a flow {tuple(t.shape)} on a chain of {self.shape}")
            jobs = [(fw, st, r.forward, r.occ_forward, fw, st)]
            if self._both:
                c, n = self._cur, 1 - self._cur
                jobs.append((r.backward, r.occ_backward, self._bw[c], self._bw_state[c], self._bw[n], self._bw_state[n]))
            self._lib.flow_compose(jobs)
            if self._both:
                self._cur = 1 - self._cur
        else:
            _flow4(r, "FlowChain.push")
            if tuple(r.shape) != self.shape:
                raise PfError(f"FlowChain.push: a flow {tuple(r.shape)} on a chain of {self.shape}")
            self._lib.flow_compose([(fw, st, r, None, fw, st)])
            self._both = False
        self.length += 1
        return self

    @property
    def forward(self) -> torch.Tensor:
        """flow(anchor -> latest frame) on the anchor's grid [B,2,H,W]; u keeps its winding."""
        return self._fw

    @property
    def state(self) -> torch.Tensor:
        """The state bytes of ``forward`` [B,H,W]."""
        return self._fw_state

    @property
    def visible(self) -> torch.Tensor:
        """bool [B,H,W]: state == 0."""
        return self._fw_state == 0

    @property
    def backward(self) -> Optional[torch.Tensor]:
        """flow(latest frame -> anchor) on the latest frame's grid, or None after a plain flow was pushed."""
        return self._bw[self._cur] if self._both else None

    @property
    def backward_state(self) -> Optional[torch.Tensor]:
        return self._bw_state[self._cur] if self._both else None


class PointTracker:
    """B x N points carried through the flows of consecutive pairs.  points [B,N,2] = (x, y) in pixels of an H x W panorama.
    ``push(flow, occ=None)`` -> (pos, state): pos <- pos + g^(pos) in place, x unwrapped (it winds), state uint8 [B,N] sticky.
    ``history=T`` keeps the last T positions in a device ring [T,B,N,2] (``trajectory()`` orders them)."""

    def __init__(self, points: torch.Tensor, H: int, W: int, history: Optional[int] = None, lib=None):
        if not isinstance(points, torch.Tensor) or points.dim() != 3 or points.shape[2] != 2 or points.shape[1] < 1:
            raise PfError("PointTracker: points must be a tensor [B,N,2] of (x, y) pixels")
        self._lib = _library(points.device, lib)
        if min(H, W) < 1 or (history is not None and history < 1):
            raise PfError(f"PointTracker: H, W = {H}, {W}, history = {history}")
        self.H, self.W = int(H), int(W)
        self.pos = points.detach().float().contiguous().clone()
        self.state = torch.zeros(points.shape[:2], dtype=torch.uint8, device=points.device)
        self._ring = None if history is None else torch.zeros(history, *self.pos.shape, dtype=torch.float32, device=points.device)
        self.steps = 0

    @classmethod
    def grid(cls, B: int, H: int, W: int, device, history: Optional[int] = None, lib=None) -> "PointTracker":
        """A tracker on every pixel centre (pf_track_grid): point y * W + x of each image starts at (x, y)."""
        t = cls(torch.zeros(B, H * W, 2, device=device), H, W, history=history, lib=lib)
        t._lib.track_grid(t.pos, H, W)
        return t

    def push(self, flow: torch.Tensor, occ: Optional[torch.Tensor] = None):
        _flow4(flow, "PointTracker.push")
        if tuple(flow.shape) != (self.pos.shape[0], 2, self.H, self.W):
            raise PfError(f"PointTracker.push: flow {tuple(flow.shape)}, expected {(self.pos.shape[0], 2, self.H, self.W)}")
        self._lib.track_points(self.pos, self.state, flow, occ)
        if self._ring is not None:
            self._ring[self.steps % self._ring.shape[0]].copy_(self.pos)
        self.steps += 1
        return self.pos, self.state

    @property
    def pos_wrapped(self) -> torch.Tensor:
        """The positions with x taken modulo W (a copy)."""
        out = self.pos.clone()
        out[..., 0] = torch.remainder(out[..., 0], float(self.W))
        return out

    @property
    def history(self) -> Optional[torch.Tensor]:
        """The ring [T,B,N,2]: step s (counted from 0) sits in slot s % T."""
        return self._ring

    def trajectory(self) -> torch.Tensor:
        """The kept positions, oldest first: [min(steps, T),B,N,2] (a copy)."""
        if self._ring is None:
            raise PfError("PointTracker: built without history")
        T = self._ring.shape[0]
        k = min(self.steps, T)
        idx = [(self.steps - k + i) % T for i in range(k)]
        return self._ring[idx]
