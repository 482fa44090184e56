"""Depth along the trajectory on the device: rigid reprojection of an inverse-depth panorama into the next camera, a z-tested
forward splat and a per-pixel recursive depth filter.

    stream = FlowStream(model, iters=12, bidirectional=True, occlusion="sphere")
    odo = Odometry(B, H, W, device)
    prop = DepthPropagator(odo)
    for frame in frames:
        r = stream(frame)
        if r is not None:
            odo.push(r)
            prop.push()
            prop.inv_depth, prop.weight                 # of the pair's EARLIER frame, filtered over the segment so far
            prop.rigid_flow, prop.predicted_inv_depth   # what depth and pose predict for the flow, and the LATER frame's depth

The convention is section 20's point motion: a scene point X in the earlier frame's axes is R X + T in the later frame's, T in the
unit of the inverse depth (``T = odo.baseline[:, None] * odo.pose.t``, a device tensor).  ``rigid_flow`` is the flow a static scene
of that depth shows under that pose; the network's flow minus it is independent motion in pixels.  ``reproject`` moves the depth
map (and up to four payload planes, e.g. the frame) into the later camera: of the samples that land on a pixel only those within
2^ztol_log2 of the nearest one are blended, so a foreground surface hides what lies behind it.  There is no CPU path: tensors on
the host are refused (PfError).

b_min = 0.25, ztol_log2 = 0.25, tol_log2 = 0.5, decay = 0.9, w_max = 8, cmin = 0.5, n_min = 1e-6 and dmax = 2^16 are choices, not
measurements (DESIGN.md section 23 says what they were tried on).
"""
from __future__ import annotations

import math

import torch

from ._lib import PfError
from .egomotion import _device, _fit, _library, _on
from .inpaint import HoleFiller
from .odometry import Odometry

DEFAULTS = dict(b_min=0.25, ztol_log2=0.25, w_max=8.0, cmin=0.5, n_min=1e-6, dmax=65536.0, vmax=255.0)
_FILTER_DEFAULTS = dict(tol_log2=0.5, decay=0.9)


def _options(what, given, allowed):
    unknown = [k for k in given if k not in allowed]
    if unknown:
        raise PfError(f"{what}: unknown options {unknown}")
    try:
        o = dict(allowed, **{k: float(v) for k, v in given.items()})
    except (TypeError, ValueError):
        raise PfError(f"{what}: an option is not a number: {given}") from None
    if not all(math.isfinite(v) for v in o.values()):
        raise PfError(f"{what}: an option is not finite: {o}")
    if "b_min" in o and not (0 <= o["b_min"] <= 1 and 0 <= o["ztol_log2"] <= 64 and o["w_max"] > 0 and o["cmin"] > 0 and o["n_min"] > 0
                             and 1 <= o["dmax"] <= 65536 and 1 <= o["vmax"] <= 65536):
        raise PfError(f"{what}: {o}")
    if "tol_log2" in o and not (o["tol_log2"] > 0 and 0 < o["decay"] <= 1):
        raise PfError(f"{what}: tol_log2 {o['tol_log2']!r}, decay {o['decay']!r}")
    return o


def _pose_maps(what, inv_depth, weight, R, T, mask):
    if not isinstance(inv_depth, torch.Tensor) or inv_depth.dim() != 3:
        raise PfError(f"{what}: inv_depth must be a tensor [B,H,W]")
    B, H, W = inv_depth.shape
    dev = inv_depth.device
    _fit(inv_depth, (B, H, W), f"{what}: inv_depth", dev)
    _fit(weight, (B, H, W), f"{what}: weight", dev)
    _fit(R, (B, 3, 3), f"{what}: R", dev)
    _fit(T, (B, 3), f"{what}: T", dev)
    if mask is not None:
        _fit(mask, (B, H, W), f"{what}: mask", dev, torch.uint8)
    return B, H, W, dev


def _distinct(what, outs, ins):
    """No output may be an input or another output.  Only equal start addresses are compared here, to name the tensor; a partial
    overlap through views is left to the library's check, which refuses any overlapping bytes (PfError, without the name)."""
    seen = {}
    for name, t in ins:
        if t is not None:
            seen[t.data_ptr()] = name
    for name, t in outs:
        if t is None:
            continue
        if t.data_ptr() in seen:
            raise PfError(f"{what}: {name} aliases {seen[t.data_ptr()]}")
        seen[t.data_ptr()] = name


def rigid_flow(inv_depth, weight, R, T, mask=None, out=None, n_min: float = DEFAULTS["n_min"], lib=None):
    """(flow fp32 [B,2,H,W], d_new fp32 [B,H,W], valid uint8 [B,H,W]): where every pixel of an inverse-depth map [B,H,W] goes under
    X -> R X + T (R [B,3,3], T [B,3] device tensors) and its inverse depth seen from there.  A pixel with weight <= 0, a set mask
    byte, an inverse depth outside [0, 2^30) or a point nearer than n_min to the new centre gives flow 0, d_new 0, valid 0.
    out: the three tensors to write (default: new ones)."""
    B, H, W, dev = _pose_maps("rigid_flow", inv_depth, weight, R, T, mask)
    lib = _library(dev, lib)
    if not (n_min > 0 and math.isfinite(n_min)):
        raise PfError(f"rigid_flow: n_min = {n_min!r}")
    if out is None:
        out = (torch.empty(B, 2, H, W, dtype=torch.float32, device=dev), torch.empty(B, H, W, dtype=torch.float32, device=dev),
               torch.empty(B, H, W, dtype=torch.uint8, device=dev))
    else:
        out = tuple(out)
        if len(out) != 3:
            raise PfError("rigid_flow: out is (flow, d_new, valid)")
        _fit(out[0], (B, 2, H, W), "rigid_flow: flow", dev)
        _fit(out[1], (B, H, W), "rigid_flow: d_new", dev)
        _fit(out[2], (B, H, W), "rigid_flow: valid", dev, torch.uint8)
    _distinct("rigid_flow", (("flow", out[0]), ("d_new", out[1]), ("valid", out[2])),
              (("inv_depth", inv_depth), ("weight", weight), ("mask", mask), ("R", R), ("T", T)))
    with _on(dev):
        lib.reproj_project(inv_depth, weight, mask, R, T, out[0], out[1], out[2], n_min)
    return out


class Reprojector:
    """An inverse-depth map (and C = 0..4 payload planes) of B panoramas moved into the camera R X + T, with every buffer allocated
    here: ``run`` launches four times on the current stream (project, front, accumulate, resolve), allocates nothing, never
    synchronises and can be captured into a HIP graph.  It keeps ``flow``, ``d_new``, ``valid`` (the projection) and ``out``,
    ``inv_depth``, ``weight``, ``hole`` (the result; overwritten by the next call).  fill = True: six more launches close the holes
    of the result from its own push-pull pyramid (``inpaint.HoleFiller``) into ``filled`` (of ``out``; None when C = 0) and
    ``filled_inv_depth`` (of ``inv_depth``, with ``weight`` as the soft weight); the result itself stays as it is."""

    def __init__(self, B: int, C: int, H: int, W: int, device, lib=None, fill: bool = False, **options):
        self.lib = _library(device, lib)
        self.device = _device(device)
        if min(B, H, W) < 1 or not 0 <= C <= 4:
            raise PfError(f"Reprojector: B, C, H, W = {B}, {C}, {H}, {W} (C = 0..4)")
        self.o = _options("Reprojector", options, DEFAULTS)
        self.B, self.C, self.H, self.W = B, C, H, W
        self.lib.zsplat_bytes(B, C, H, W)                          # the geometry the library accepts
        dev = self.device
        f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)                    # noqa: E731
        self.acc = torch.zeros(B, C + 3, H, W, dtype=torch.int64, device=dev)
        self.front = torch.zeros(B, H, W, dtype=torch.int32, device=dev)
        self.flow, self.d_new = f32(B, 2, H, W), f32(B, H, W)
        self.valid = torch.zeros(B, H, W, dtype=torch.uint8, device=dev)
        self.out = f32(B, C, H, W) if C else None
        self.inv_depth, self.weight = f32(B, H, W), f32(B, H, W)
        self.hole = torch.zeros(B, H, W, dtype=torch.uint8, device=dev)
        if not isinstance(fill, bool):
            raise PfError(f"Reprojector: fill = {fill!r}, expected True or False")
        self.fill = fill
        self.filled = self.filled_inv_depth = self.frame_filler = self.depth_filler = None
        if fill:
            self.depth_filler = HoleFiller(B, 1, H, W, dev, lib=lib)
            self.filled_inv_depth = self.depth_filler.out.view(B, H, W)
            if C:
                self.frame_filler = HoleFiller(B, C, H, W, dev, lib=lib)
                self.filled = self.frame_filler.out

    def reset(self) -> None:
        """Rewrite every buffer (the sums and the front are all-zero after every completed call; this is for one cut short)."""
        with _on(self.device):
            for x in (self.acc, self.front, self.flow, self.d_new, self.valid, self.out, self.inv_depth, self.weight, self.hole,
                      self.filled, self.filled_inv_depth):
                if x is not None:
                    x.zero_()

    def splat(self, src, weight):
        """The three launches behind the projection: ``self.flow`` / ``d_new`` / ``valid`` (and src, weight) into the result."""
        o, lib = self.o, self.lib
        lib.zsplat_front(src, self.flow, self.d_new, weight, self.valid, self.front, o["b_min"])
        lib.zsplat_accumulate(src, self.flow, self.d_new, weight, self.valid, self.front, self.acc, o["b_min"], o["ztol_log2"],
                              o["w_max"], o["dmax"], o["vmax"])
        lib.zsplat_resolve(self.acc, self.front, self.out, self.inv_depth, self.weight, self.hole, o["cmin"], o["w_max"], o["dmax"],
                           o["vmax"])
        if self.fill:
            if self.frame_filler is not None:
                self.frame_filler.fill(self.out, self.hole)
            self.depth_filler.fill(self.inv_depth.view(self.B, 1, self.H, self.W), self.hole, self.weight)

    def run(self, src, inv_depth, weight, R, T, mask=None):
        """(out [B,C,H,W] or None, inv_depth, weight fp32 [B,H,W], hole uint8 [B,H,W]) in the later camera.  src: fp32 [B,C,H,W]
        on the earlier frame's grid (None when C = 0)."""
        B, C, H, W, dev = self.B, self.C, self.H, self.W, self.device
        if (src is None) != (C == 0):
            raise PfError(f"Reprojector.run: src is {'required' if C else 'not taken'} with C = {C}")
        if src is not None:
            _fit(src, (B, C, H, W), "Reprojector.run: src", dev)
        for t, shape, what, dt in ((inv_depth, (B, H, W), "inv_depth", torch.float32), (weight, (B, H, W), "weight", torch.float32),
                                   (R, (B, 3, 3), "R", torch.float32), (T, (B, 3), "T", torch.float32)):
            _fit(t, shape, f"Reprojector.run: {what}", dev, dt)
        if mask is not None:
            _fit(mask, (B, H, W), "Reprojector.run: mask", dev, torch.uint8)
        _distinct("Reprojector.run", (("out", self.out), ("inv_depth (result)", self.inv_depth), ("weight (result)", self.weight),
                                      ("hole", self.hole), ("flow", self.flow), ("d_new", self.d_new), ("valid", self.valid)),
                  (("src", src), ("inv_depth", inv_depth), ("weight", weight), ("mask", mask), ("R", R), ("T", T)))
        with _on(dev):
            self.lib.reproj_project(inv_depth, weight, mask, R, T, self.flow, self.d_new, self.valid, self.o["n_min"])
            self.splat(src, weight)
        return self.out, self.inv_depth, self.weight, self.hole


def reproject(src, inv_depth, weight, R, T, mask=None, lib=None, **options):
    """(out_src [B,C,H,W] or None, inv_depth, weight fp32 [B,H,W], hole uint8 [B,H,W]) of one map moved into the camera R X + T.
    src: fp32 [B,C,H,W] (C = 1..4) or None.  The buffers are allocated per call (for a video use ``Reprojector``)."""
    B, H, W, dev = _pose_maps("reproject", inv_depth, weight, R, T, mask)
    if src is not None and (not isinstance(src, torch.Tensor) or src.dim() != 4):
        raise PfError("reproject: src must be a tensor [B,C,H,W] or None")
    with torch.no_grad():
        rp = Reprojector(B, 0 if src is None else src.shape[1], H, W, dev, lib=lib, **options)
        return rp.run(src, inv_depth, weight, R, T, mask)


class DepthPropagator:
    """The depth of B videos carried along the path of an ``Odometry`` and fused with each new measurement, with every buffer
    allocated here.  ``push()`` is called after each ``odo.push(r)``; it runs on the current stream, reads nothing on the host,
    allocates nothing after construction and can be captured into a HIP graph:

      the state (the map predicted into the pair's earlier frame by the push before) is updated with ``odo.inv_depth`` /
      ``depth_weight`` / ``disagree`` -> ``inv_depth``, ``weight`` of the earlier frame; a change of ``odo.flags``' segment drops
      the state of that image first.  Then the filtered map is projected with ``odo.pose.R`` and T = ``odo.baseline`` *
      ``odo.pose.t`` (``odo.map_b``'s moving byte as mask) -> ``rigid_flow``, and z-splatted into the later frame's grid ->
      ``predicted_inv_depth``, ``predicted_weight``, ``hole``, the state of the next push.

    channels = 3 and ``push(frame=previous)`` (fp32 [B,3,H,W]) also give ``predicted_frame``, the earlier frame rendered from the
    later camera.  fill = True also gives ``predicted_frame_filled`` and ``predicted_inv_depth_filled``, the two with their holes
    closed (``Reprojector(fill=True)``); the state and the filter keep using the unfilled maps.  Options: ``Reprojector``'s, and
    tol_log2, decay of the filter."""

    def __init__(self, odo: Odometry, channels: int = 0, fill: bool = False, **options):
        if not isinstance(odo, Odometry):
            raise PfError("DepthPropagator: odo is an Odometry")
        if channels not in (0, 1, 2, 3, 4):
            raise PfError(f"DepthPropagator: channels = {channels!r}, expected 0..4")
        self.odo, self.lib, self.device = odo, odo.lib, odo.device
        self.B, self.H, self.W, self.C = odo.B, odo.H, odo.W, int(channels)
        self.f = _options("DepthPropagator", {k: v for k, v in options.items() if k in _FILTER_DEFAULTS}, _FILTER_DEFAULTS)
        self.rp = Reprojector(self.B, self.C, self.H, self.W, self.device, lib=self.lib, fill=fill,
                              **{k: v for k, v in options.items() if k not in _FILTER_DEFAULTS})
        B, H, W, dev = self.B, self.H, self.W, self.device
        self.inv_depth = torch.zeros(B, H, W, dtype=torch.float32, device=dev)
        self.weight = torch.zeros(B, H, W, dtype=torch.float32, device=dev)
        self.seg = torch.zeros(B, dtype=torch.int32, device=dev)
        self.T = torch.zeros(B, 3, dtype=torch.float32, device=dev)
        self.rigid_flow, self.valid = self.rp.flow, self.rp.valid
        self.predicted_inv_depth, self.predicted_weight, self.hole = self.rp.inv_depth, self.rp.weight, self.rp.hole
        self.predicted_frame = self.rp.out
        self.predicted_frame_filled, self.predicted_inv_depth_filled = self.rp.filled, self.rp.filled_inv_depth
        self.reset()

    def reset(self) -> None:
        """Forget the depth: the next push starts from its measurement alone.  Every buffer is rewritten."""
        with _on(self.device):
            self.rp.reset()
            for x in (self.inv_depth, self.weight, self.seg, self.T):
                x.zero_()

    def push(self, frame=None):
        """One pair, after ``odo.push``: (inv_depth, weight) fp32 [B,H,W] of the pair's earlier frame, filtered."""
        odo, lib, rp, dev = self.odo, self.lib, self.rp, self.device
        if (frame is None) != (self.C == 0):
            raise PfError(f"DepthPropagator.push: frame is {'required' if self.C else 'not taken'} with channels = {self.C}")
        if frame is not None:
            _fit(frame, (self.B, self.C, self.H, self.W), "DepthPropagator.push: frame", dev)
        with _on(dev):
            self.inv_depth.copy_(rp.inv_depth)
            self.weight.copy_(rp.weight)
            lib.depth_update(self.inv_depth, self.weight, odo.inv_depth, odo.depth_weight, odo.disagree, odo.flags, self.seg,
                             self.f["tol_log2"], self.f["decay"], rp.o["w_max"])
            torch.mul(odo.baseline.unsqueeze(1), odo.pose.t, out=self.T)
            lib.reproj_project(self.inv_depth, self.weight, odo.map_b[3], odo.pose.R, self.T, rp.flow, rp.d_new, rp.valid, rp.o["n_min"])
            rp.splat(frame, self.weight)
        return self.inv_depth, self.weight
