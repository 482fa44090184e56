"""Forward warping on the device: softmax splatting and frame interpolation.

    stream = FlowStream(model, iters=12, bidirectional=True, occlusion="sphere")
    interp = FrameInterpolator(B, 3, H, W, device)
    prev = None
    for frame in frames:
        r = stream(frame)
        if r is not None:
            mid, hole = interp.from_bidirectional(r, prev, frame, 0.5)     # two launches behind the step, capturable
        prev = frame

    out, hole = splat(src, flow, tau=1.0)          # any map [B,C,H,W] moved along its own flow, e.g. along FlowChain.forward

Every other mover of this package GATHERS (each output pixel samples where its flow points); this one SCATTERS: source pixel
(x, y) lands at (x + tau u, y + tau v), spread over the four pixels around it (columns wrap, a row past a pole is dropped), with
the weight beta * exp(-min(alpha * m, zmax)) of its importance metric m; a target pixel is the weighted mean of what reached it
(softmax splatting), a pixel that too little reached (coverage below ``cmin``) is a hole.  The sums are 64-bit integers
(``csrc/pf_splat.h``), so the result is the same bits on every run and under every launch order.  There is no CPU path: tensors on
the host are refused (PfError).
"""
from __future__ import annotations

import contextlib
from typing import Optional

import torch

from . import _lib
from ._lib import PfError
from .inpaint import HoleFiller
from .video import BidirectionalFlow


def _library(device, lib):
    """The product's library for a cuda/ROCm device; `lib` (a handle of the tests' host emulation) lifts the device rule."""
    if lib is not None:
        return lib
    if torch.device(device).type != "cuda":
        raise PfError("softmax splatting needs tensors on a cuda/ROCm device; there is no CPU fallback")
    return _lib.load()


def _fit(t, shape, what: str, device, dtype=torch.float32):
    """A contiguous tensor of exactly this dtype, shape and device: nothing is converted or copied behind the caller's back."""
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_contiguous() or tuple(t.shape) != tuple(shape) \
            or t.device != device:
        got = f"{t.dtype} {tuple(t.shape)} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise PfError(f"{what} must be a contiguous {dtype} tensor {tuple(shape)} on {device}, got {got}")
    return t


def _fit_metric(t, B, H, W, what, device):
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or t.dim() != 4 or t.shape[1] not in (1, 2):
        raise PfError(f"{what} must be [B,1,H,W] or [B,2,H,W]")
    return _fit(t, (B, t.shape[1], H, W), what, device)


def splat(src: torch.Tensor, flow: torch.Tensor, tau: float = 1.0, metric: Optional[torch.Tensor] = None,
          mask: Optional[torch.Tensor] = None, alpha: float = 0.0, vmax: float = 255.0, zmax: float = 12.0, cmin: float = 2.0 ** -10,
          lib=None):
    """(out [B,C,H,W], hole uint8 [B,H,W]) of one map moved along its own flow: src fp32 [B,C,H,W] (C = 1..4, values clamped to
    +-vmax), flow [B,2,H,W] on the same grid, tau how far along it.  metric [B,1|2,H,W] and alpha weigh the samples that meet in a
    pixel by exp(-alpha * |metric|); mask uint8 [B,H,W]: non-zero pixels are left out.  A hole is 0.  The buffers are allocated
    per call (for a video use ``FrameInterpolator``)."""
    if not isinstance(src, torch.Tensor) or src.dim() != 4:
        raise PfError("splat: src must be a tensor [B,C,H,W]")
    lib = _library(src.device, lib)
    B, C, H, W = src.shape
    dev = src.device
    _fit(src, (B, C, H, W), "splat: src", dev)
    _fit(flow, (B, 2, H, W), "splat: flow", dev)
    metric = _fit_metric(metric, B, H, W, "splat: metric", dev)
    if mask is not None:
        _fit(mask, (B, H, W), "splat: mask", dev, torch.uint8)
    with torch.no_grad():
        acc = torch.zeros(B, C + 2, H, W, dtype=torch.int64, device=dev)
        out = torch.empty(B, C, H, W, dtype=torch.float32, device=dev)
        hole = torch.empty(B, H, W, dtype=torch.uint8, device=dev)
        lib.splat_accumulate([(src, flow, metric, mask, tau, 1.0)], acc, alpha, zmax, vmax)
        lib.splat_resolve(acc, out, hole, 1, vmax, cmin)
    return out, hole


class FrameInterpolator:
    """The frame at time t in (0, 1) between two frames of B videos from the two flows between them, with every buffer allocated
    here: ``frame`` launches twice on the current stream (accumulate, resolve), allocates nothing, never synchronises and can be
    captured into a HIP graph together with a ``FlowStream`` step.

    Frame 0 is moved along flow01 by t with blend weight 1 - t, frame 1 along flow10 by 1 - t with blend weight t; a sample's
    importance is exp(-min(alpha * m, zmax)) of its metric m.  alpha is a choice, not a measurement: at alpha * |residual| = 1
    a sample counts e^-1 against one whose round trip closes, so the default 1.0 discounts a sample by e per pixel of
    forward-backward residual.  A target pixel whose coverage (the blend weights that reached it, without the importance) is
    below ``cmin`` is a hole: with fill "blend" it takes (1 - t) frame0 + t frame1 and stays flagged, with "none" it is 0, with
    "pushpull" it is resolved as with "none" and then filled in place from the frame's own pyramid (``inpaint.HoleFiller``,
    three more launches); ``hole`` stays as flagged.
    Values are clamped to +-vmax (declare the range of the frames: it fixes the scale of the integer sums)."""

    FILLS = ("blend", "none", "pushpull")

    def __init__(self, B: int, C: int, H: int, W: int, device, alpha: float = 1.0, zmax: float = 12.0, cmin: float = 2.0 ** -10,
                 vmax: float = 255.0, fill: str = "blend", lib=None):
        self.lib = _library(device, lib)
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if fill not in self.FILLS:
            raise PfError(f"FrameInterpolator: fill {fill!r}, expected one of {self.FILLS}")
        if min(B, H, W) < 1 or not 1 <= C <= 4:
            raise PfError(f"FrameInterpolator: B, C, H, W = {B}, {C}, {H}, {W} (C = 1..4)")
        if not (alpha >= 0 and zmax >= 0 and cmin > 0 and 1 <= vmax <= 65536):
            raise PfError(f"FrameInterpolator: alpha {alpha!r}, zmax {zmax!r}, cmin {cmin!r}, vmax {vmax!r}")
        self.B, self.C, self.H, self.W = B, C, H, W
        self.alpha, self.zmax, self.cmin, self.vmax, self.fill = float(alpha), float(zmax), float(cmin), float(vmax), fill
        self.lib.splat_scratch_bytes(B, C, H, W)                   # the geometry the library accepts
        self.acc = torch.zeros(B, C + 2, H, W, dtype=torch.int64, device=self.device)
        self.out = torch.zeros(B, C, H, W, dtype=torch.float32, device=self.device)
        self.hole = torch.zeros(B, H, W, dtype=torch.uint8, device=self.device)
        self.filler = HoleFiller(B, C, H, W, self.device, lib=lib) if fill == "pushpull" else None

    def reset(self) -> None:
        """Zero the sums again (they are all-zero after every completed call; this is for a call that was cut short)."""
        self.acc.zero_()

    def frame(self, frame0, frame1, flow01, flow10, t: float, metric0=None, metric1=None, mask0=None, mask1=None, out=None):
        """(frame_t [B,C,H,W], hole uint8 [B,H,W]).  flow01: frame 0 -> frame 1 on frame 0's grid, flow10 the other way on frame
        1's; metric0 / mask0 belong to frame 0's pixels (e.g. ``residual_forward`` / ``occ_forward``), metric1 / mask1 to frame
        1's.  out: where to write the frame (default: ``self.out``); it must not be one of the frames."""
        B, C, H, W, dev = self.B, self.C, self.H, self.W, self.device
        t = float(t)
        if not 0.0 < t < 1.0:
            raise PfError(f"FrameInterpolator.frame: t = {t!r} outside (0, 1)")
        _fit(frame0, (B, C, H, W), "frame0", dev)
        _fit(frame1, (B, C, H, W), "frame1", dev)
        _fit(flow01, (B, 2, H, W), "flow01", dev)
        _fit(flow10, (B, 2, H, W), "flow10", dev)
        metric0 = _fit_metric(metric0, B, H, W, "metric0", dev)
        metric1 = _fit_metric(metric1, B, H, W, "metric1", dev)
        for m, what in ((mask0, "mask0"), (mask1, "mask1")):
            if m is not None:
                _fit(m, (B, H, W), what, dev, torch.uint8)
        out = self.out if out is None else _fit(out, (B, C, H, W), "out", dev)
        if out.data_ptr() in (frame0.data_ptr(), frame1.data_ptr()):
            raise PfError("FrameInterpolator.frame: out must not be one of the frames")
        fills = (frame0, frame1) if self.fill == "blend" else (None, None)
        with torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext():
            self.lib.splat_accumulate([(frame0, flow01, metric0, mask0, t, 1.0 - t), (frame1, flow10, metric1, mask1, 1.0 - t, t)],
                                      self.acc, self.alpha, self.zmax, self.vmax)
            self.lib.splat_resolve(self.acc, out, self.hole, 2, self.vmax, self.cmin, fills[0], fills[1], t)
            if self.filler is not None:
                self.filler.fill(out, self.hole, out=out)
        return out, self.hole

    def from_bidirectional(self, r: BidirectionalFlow, frame0, frame1, t: float, importance: Optional[str] = "residual",
                           use_occlusion: bool = False, out=None):
        """``frame`` on what a bidirectional ``FlowStream`` returned for the pair (frame0, frame1).  importance "residual": the
        forward-backward residuals are the metrics (None: every sample counts alike); use_occlusion: the occlusion masks leave
        their pixels out altogether."""
        if not isinstance(r, BidirectionalFlow):
            raise PfError("FrameInterpolator.from_bidirectional: r is what a bidirectional FlowStream returns")
        if importance not in ("residual", None):
            raise PfError(f"FrameInterpolator.from_bidirectional: importance {importance!r}, expected 'residual' or None")
        m0 = m1 = k0 = k1 = None
        if importance == "residual":
            m0, m1 = r.residual_forward, r.residual_backward
            if m0 is None or m1 is None:
                raise PfError("FrameInterpolator.from_bidirectional: the stream ran without occlusion=..., so it has no residuals")
        if use_occlusion:
            k0, k1 = r.occ_forward, r.occ_backward
            if k0 is None or k1 is None:
                raise PfError("FrameInterpolator.from_bidirectional: the stream ran without occlusion=..., so it has no masks")
        return self.frame(frame0, frame1, r.forward, r.backward, t, m0, m1, k0, k1, out=out)
