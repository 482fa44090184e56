"""Camera rotation from 360-degree flow on the device, and video stabilisation.

    stream = FlowStream(model, iters=12, bidirectional=True, occlusion="sphere")
    stab = Stabilizer(B, 3, H, W, device, smoothing=0.9)
    for frame in frames:
        r = stream(frame)
        if r is not None:
            steady = stab.push_bidirectional(r, frame)      # 2 * passes + 2 launches behind the step, capturable
            R = stab.estimator.R                            # the camera's rotation for this pair, [B,3,3] on the device
            rest = derotate_flow(r.forward, R)              # what is left: parallax and independent motion

On the sphere a camera rotation is one rigid motion of every bearing, so it can be read off a full-sphere flow field in closed
form (Horn's quaternion solution), with no focal length and no field-of-view loss; the corrected frame is again a complete
panorama.  A pixel of the flow says that the bearing p = s(x, y) of the earlier frame is seen at q = s(x + u, y + v) in the later
one; the rotation returned has q ~ R p.  The fit weighs a pixel by its solid angle and, after the first pass, by the
Geman-McClure weight of its residual, so a moving object or a region of bad flow does not drag the camera with it.  The sums are
64-bit integers (``csrc/pf_egomotion.h``): the same bits on every run.  There is no CPU path: tensors on the host are refused
(PfError).
"""
from __future__ import annotations

import contextlib
from typing import Optional

import torch

from . import _lib
from ._lib import PfError
from .video import BidirectionalFlow


def _library(device, lib):
    """The product's library for a cuda/ROCm device; `lib` (a handle of the tests' host emulation) lifts the device rule."""
    if lib is not None:
        return lib
    if torch.device(device).type != "cuda":
        raise PfError("rotation estimation needs tensors on a cuda/ROCm device; there is no CPU fallback")
    return _lib.load()


def _fit(t, shape, what: str, device, dtype=torch.float32):
    """A contiguous tensor of exactly this dtype, shape and device: nothing is converted or copied behind the caller's back."""
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_contiguous() or tuple(t.shape) != tuple(shape) \
            or t.device != device:
        got = f"{t.dtype} {tuple(t.shape)} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise PfError(f"{what} must be a contiguous {dtype} tensor {tuple(shape)} on {device}, got {got}")
    return t


def _device(device) -> torch.device:
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def _on(dev):
    return torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext()


def _eye(B, device):
    return torch.eye(3, dtype=torch.float32, device=device).repeat(B, 1, 1).contiguous()


class RotationEstimator:
    """The rotation R [B,3,3] with q ~ R p of B flow fields [B,2,H,W], with every buffer allocated here: ``estimate`` launches
    2 * passes kernels (and one fill of 96 B bytes) on the current stream, allocates nothing, never synchronises and can be captured
    into a HIP graph together with a ``FlowStream`` step.

    Pass 0 is the plain solid-angle-weighted fit; each further pass weighs a pixel by 1 / (1 + r^2 / c^2)^2 of its chord r under
    the rotation of the pass before, c = scale_px pixel widths at the equator.  passes = 4 and scale_px = 1.0 are choices, not
    measurements (DESIGN.md section 19 says what they were tried on), and so is gap_min = 1e-3: ``stats[:, 4]`` (valid) is 0 when
    nothing was left to fit or the two largest eigenvalues of the fit lie closer than gap_min of the weight, and R is then
    ``init`` (the identity without one).  ``stats`` [B,5] = {sum of weights, rms chord of the last pass, used fraction, gap,
    valid}."""

    def __init__(self, B: int, H: int, W: int, device, passes: int = 4, scale_px: float = 1.0, gap_min: float = 1e-3, lib=None,
                 blocks: int = 0):
        self.lib = _library(device, lib)
        self.device = _device(device)
        if min(B, H, W) < 1:
            raise PfError(f"RotationEstimator: B, H, W = {B}, {H}, {W}")
        if int(passes) != passes or passes < 1:
            raise PfError(f"RotationEstimator: passes = {passes!r}, expected an integer >= 1")
        if not (scale_px > 0 and gap_min >= 0 and 0 <= blocks <= 65535):
            raise PfError(f"RotationEstimator: scale_px {scale_px!r}, gap_min {gap_min!r}, blocks {blocks!r}")
        self.B, self.H, self.W = B, H, W
        self.passes, self.scale_px, self.gap_min, self.blocks = int(passes), float(scale_px), float(gap_min), int(blocks)
        self.lib.ego_scratch_bytes(B, H, W)                        # the geometry the library accepts
        self.sums = torch.zeros(B, _lib.EGO_SUMS, dtype=torch.int64, device=self.device)
        self.R = _eye(B, self.device)
        self.stats = torch.zeros(B, _lib.EGO_STATS, dtype=torch.float32, device=self.device)
        self.identity = _eye(B, self.device)

    def estimate(self, flow, mask=None, init=None):
        """R [B,3,3] (``self.R``, overwritten by the next call).  flow fp32 [B,2,H,W]; mask uint8 [B,H,W]: non-zero pixels are left
        out (e.g. ``occ_forward``), as are pixels whose flow is not finite; init [B,3,3]: where the reweighting starts from and
        what an invalid fit returns (default: the identity)."""
        B, H, W, dev = self.B, self.H, self.W, self.device
        _fit(flow, (B, 2, H, W), "flow", dev)
        if mask is not None:
            _fit(mask, (B, H, W), "mask", dev, torch.uint8)
        init = self.identity if init is None else _fit(init, (B, 3, 3), "init", dev)
        if init.data_ptr() == self.R.data_ptr():
            raise PfError("RotationEstimator.estimate: init must not be the estimator's own R (clone it)")
        with _on(dev):
            self.sums.zero_()                                      # all-zero after every completed call; a cut-short one costs nothing
            for k in range(self.passes):
                self.lib.ego_accumulate(flow, mask, init if k == 0 else self.R, self.sums, k > 0, self.scale_px, self.blocks)
                self.lib.ego_solve(self.sums, init, self.R, self.stats, H, W, self.gap_min)
        return self.R


def derotate_flow(flow, R, valid=None, mask=None, out=None, lib=None):
    """The flow with the rotation R removed: flow'(x, y) = erp(R^T q) - (x, y), u' wrapped into [-W/2, W/2).  What is left of a
    static scene is parallax.  flow fp32 [B,2,H,W], R [B,3,3]; valid uint8 [B,H,W] (optional) is cleared where the pixel was left
    out (masked by ``mask``, or a flow that is not finite), and the flow is (0, 0) there.  out: where to write (default: a new
    tensor; it may be ``flow``)."""
    if not isinstance(flow, torch.Tensor) or flow.dim() != 4:
        raise PfError("derotate_flow: flow must be a tensor [B,2,H,W]")
    lib = _library(flow.device, lib)
    B, _, H, W = flow.shape
    dev = flow.device
    _fit(flow, (B, 2, H, W), "derotate_flow: flow", dev)
    _fit(R, (B, 3, 3), "derotate_flow: R", dev)
    for m, what in ((valid, "valid"), (mask, "mask")):
        if m is not None:
            _fit(m, (B, H, W), f"derotate_flow: {what}", dev, torch.uint8)
    out = torch.empty_like(flow) if out is None else _fit(out, (B, 2, H, W), "derotate_flow: out", dev)
    with _on(dev):
        lib.ego_derotate(flow, mask, R, out, valid)
    return out


def rotate_erp(frame, R, out=None, lib=None):
    """out(x, y) = frame sampled at erp(R s(x, y)) (four taps, columns wrap, rows clamp): frame fp32 [B,C,H,W] or uint8 [B,H,W,C],
    C = 1..4, R [B,3,3] on the device.  With R = ``Stabilizer.correction`` this is the stabilised frame."""
    if not isinstance(frame, torch.Tensor) or frame.dim() != 4 or frame.dtype not in (torch.float32, torch.uint8):
        raise PfError("rotate_erp: frame must be a tensor fp32 [B,C,H,W] or uint8 [B,H,W,C]")
    lib = _library(frame.device, lib)
    dev = frame.device
    C = frame.shape[1] if frame.dtype == torch.float32 else frame.shape[3]
    if not 1 <= C <= 4:
        raise PfError(f"rotate_erp: {C} channels, expected 1..4")
    _fit(frame, frame.shape, "rotate_erp: frame", dev, frame.dtype)
    _fit(R, (frame.shape[0], 3, 3), "rotate_erp: R", dev)
    out = torch.empty_like(frame) if out is None else _fit(out, frame.shape, "rotate_erp: out", dev, frame.dtype)
    if out.data_ptr() == frame.data_ptr():
        raise PfError("rotate_erp: out must not be the frame")
    with _on(dev):
        lib.erp_rotate(frame, R, out)
    return out


class Stabilizer:
    """Rotation-stabilised video: ``push(frame, flow)`` takes frame t and the flow from frame t-1 to it (on frame t-1's grid),
    estimates the camera's rotation R_t, advances the orientation O_t = R_t O_{t-1} and the smoothed virtual path
    S_t = slerp(S_{t-1}, O_t, 1 - smoothing) on the device and returns frame t resampled under the correction C_t = O_t S_t^T.
    smoothing = 1 locks the view to the first frame, 0 leaves the video as it is.  Everything is launched on the current stream
    (2 * passes + 2 kernels), nothing is read on the host, nothing is allocated: a push can be captured together with the
    ``FlowStream`` step before it.  form "f32": frames fp32 [B,C,H,W]; "u8": uint8 [B,H,W,C]; C = 1..4.  The first frame of a
    video needs no push: it is its own stabilised frame."""

    FORMS = ("f32", "u8")

    def __init__(self, B: int, C: int, H: int, W: int, device, smoothing: float = 1.0, form: str = "f32", lib=None, **estimator):
        if form not in self.FORMS:
            raise PfError(f"Stabilizer: form {form!r}, expected 'f32' or 'u8'")
        if not 1 <= C <= 4:
            raise PfError(f"Stabilizer: C = {C}, expected 1..4")
        if not 0.0 <= smoothing <= 1.0:
            raise PfError(f"Stabilizer: smoothing = {smoothing!r} outside [0, 1]")
        self.estimator = RotationEstimator(B, H, W, device, lib=lib, **estimator)
        self.lib, self.device = self.estimator.lib, self.estimator.device
        self.B, self.C, self.H, self.W, self.smoothing, self.form = B, C, H, W, float(smoothing), form
        self.shape = (B, C, H, W) if form == "f32" else (B, H, W, C)
        self.dtype = torch.float32 if form == "f32" else torch.uint8
        self.state = torch.zeros(B, _lib.EGO_STATE, dtype=torch.float64, device=self.device)
        self.orientation = _eye(B, self.device)
        self.correction = _eye(B, self.device)
        self.out = torch.zeros(self.shape, dtype=self.dtype, device=self.device)
        self.reset()

    def reset(self) -> None:
        """Start a new video: the next push is relative to the frame before it."""
        self.state.zero_()
        self.state[:, 0::4] = 1.0
        self.orientation.copy_(self.estimator.identity)
        self.correction.copy_(self.estimator.identity)

    def push(self, frame, flow, mask=None, out=None):
        """The stabilised frame (``self.out`` unless ``out`` is given; it must not be the frame)."""
        _fit(frame, self.shape, "frame", self.device, self.dtype)
        out = self.out if out is None else _fit(out, self.shape, "out", self.device, self.dtype)
        if out.data_ptr() == frame.data_ptr():
            raise PfError("Stabilizer.push: out must not be the frame")
        R = self.estimator.estimate(flow, mask)
        with _on(self.device):
            self.lib.ego_track(R, self.state, self.orientation, self.correction, self.smoothing)
            self.lib.erp_rotate(frame, self.correction, out)
        return out

    def push_bidirectional(self, r: BidirectionalFlow, frame, out=None):
        """``push`` on what a bidirectional ``FlowStream`` returned for the pair that ends with ``frame``: its forward flow, with
        the pixels of its forward occlusion mask (when the stream computes one) left out."""
        if not isinstance(r, BidirectionalFlow):
            raise PfError("Stabilizer.push_bidirectional: r is what a bidirectional FlowStream returns")
        return self.push(frame, r.forward, r.occ_forward, out=out)
