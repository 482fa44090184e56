"""Camera translation from 360-degree flow on the device: the epipole, inverse depth up to the baseline and a mask of what moves
against the static scene.

    stream = FlowStream(model, iters=12, bidirectional=True, occlusion="sphere")
    pose = PoseEstimator(B, H, W, device)
    for frame in frames:
        r = stream(frame)
        if r is not None:
            R, t = pose.estimate_bidirectional(r)            # 2 * 4 + 18 launches behind the step, capturable
            inv_depth, resid, conf, moving = parallax_map(r.forward, R, t, mask=r.occ_forward)

A pixel of the flow says that the bearing p = s(x, y) of the earlier frame is seen at q = s(x + u, y + v) in the later one.  The
model is q ~ R p + kappa t with t a unit vector and kappa = |T| / depth >= 0.  This is the point-motion convention: a point of the
scene moves by T = |T| t in the second frame's axes; the camera centre itself moves along -R^T t in the first frame's axes.  On a
full sphere none of this needs intrinsics and the field of view never loses the epipole, which is a point of the image:
``erp(t)`` is where the scene flows towards, ``erp(-t)`` where it comes from.  Scale is not observable: inv_depth is |T| / depth.
The sums are 64-bit integers (``csrc/pf_epipolar.h``): the same bits on every run.  There is no CPU path: tensors on the host are
refused (PfError).
"""
from __future__ import annotations

import torch

from . import _lib
from ._lib import PfError
from .egomotion import RotationEstimator, _fit, _library, _on
from .video import BidirectionalFlow


class PoseEstimator:
    """Rotation R [B,3,3] and unit translation t [B,3] with q ~ R p + kappa t of B flow fields [B,2,H,W], every buffer allocated
    here.  It owns a ``RotationEstimator`` (``.estimator``, configured by ``**rotation``) whose answer starts the schedule and
    stays in ``.estimator.R``.

    The schedule is ``rounds`` x (``t_passes`` translation passes) with one rotation-refinement pass between consecutive rounds; a
    pass is an accumulate and a solve.  A translation pass weighs a pixel by its solid angle and by 1 / (1 + e^2 / c^2)^2 of its
    distance e from its epipolar great circle under the t of the pass before (c = scale_px pixel widths; only the very first pass
    runs with t = 0, where every weight is the solid angle), and lets it vote with its epipolar-plane normal scaled by
    |n| / sqrt(|n|^2 + c_v^2), c_v = vote_px pixel widths.  The refinement pass solves for the small rotation about the current t
    that brings the normals back onto the plane through t.

    ``stats`` [B,6] = {sum of weights, rms e in pixel widths, used fraction, gap = (l2 - l1) / (l1 + l2 + l3) of the vote matrix,
    parallax rms in pixel widths, valid}.  valid = 0 when nothing was left to fit, the gap is below gap_min or the parallax rms
    below min_parallax_px: a pure rotation (or rest) has no epipole.  t is then ``init_t`` (the zero vector without one) and R the
    rotation estimate, untouched.

    t_passes = 4, rounds = 2, scale_px = 1.0, vote_px = 0.25, gap_min = 1e-3 and min_parallax_px = 0.05 are choices, not
    measurements (DESIGN.md section 20 says what they were tried on)."""

    def __init__(self, B: int, H: int, W: int, device, t_passes: int = 4, rounds: int = 2, scale_px: float = 1.0,
                 vote_px: float = 0.25, gap_min: float = 1e-3, min_parallax_px: float = 0.05, lib=None, blocks: int = 0, **rotation):
        self.estimator = RotationEstimator(B, H, W, device, lib=lib, blocks=blocks, **rotation)
        self.lib, self.device = self.estimator.lib, self.estimator.device
        for name, v in (("t_passes", t_passes), ("rounds", rounds)):
            if int(v) != v or v < 1:
                raise PfError(f"PoseEstimator: {name} = {v!r}, expected an integer >= 1")
        if not (scale_px > 0 and vote_px > 0 and gap_min >= 0 and min_parallax_px >= 0):
            raise PfError(f"PoseEstimator: scale_px {scale_px!r}, vote_px {vote_px!r}, gap_min {gap_min!r}, "
                          f"min_parallax_px {min_parallax_px!r}")
        self.B, self.H, self.W, self.blocks = B, H, W, int(blocks)
        self.t_passes, self.rounds = int(t_passes), int(rounds)
        self.scale_px, self.vote_px, self.gap_min, self.min_parallax_px = float(scale_px), float(vote_px), float(gap_min), float(min_parallax_px)
        self.lib.epi_sums_bytes(B, H, W)                           # the geometry the library accepts
        self.sums = torch.zeros(B, _lib.EPI_SUMS, dtype=torch.int64, device=self.device)
        self.R = self.estimator.identity.clone()
        self.t = torch.zeros(B, 3, dtype=torch.float32, device=self.device)
        self.stats = torch.zeros(B, _lib.EPI_STATS, dtype=torch.float32, device=self.device)

    def estimate(self, flow, mask=None, init_R=None, init_t=None):
        """(R [B,3,3], t [B,3]) (``self.R``, ``self.t``, overwritten by the next call).  flow fp32 [B,2,H,W]; mask uint8 [B,H,W]:
        non-zero pixels are left out (e.g. ``occ_forward``), as are pixels whose flow is not finite; init_R [B,3,3]: as
        ``RotationEstimator.estimate``'s init; init_t [B,3]: what an invalid fit returns (default: the zero vector)."""
        B, H, W, dev, lib = self.B, self.H, self.W, self.device, self.lib
        if init_t is not None:
            _fit(init_t, (B, 3), "init_t", dev)
            if init_t.data_ptr() == self.t.data_ptr():
                raise PfError("PoseEstimator.estimate: init_t must not be the estimator's own t (clone it)")
        R0 = self.estimator.estimate(flow, mask, init_R)           # checks flow and mask
        with _on(dev):
            self.R.copy_(R0)
            self.sums.zero_()                                     # all-zero after every completed call; a cut-short one costs nothing
            first = True
            for rnd in range(self.rounds):
                if rnd:
                    lib.epi_accumulate(flow, mask, self.R, self.t, self.sums, _lib.EPI_R, self.scale_px, self.vote_px, self.blocks)
                    lib.epi_solve(self.sums, init_t, self.R, self.t, self.stats, H, W, _lib.EPI_R, self.gap_min, self.min_parallax_px)
                for _ in range(self.t_passes):
                    lib.epi_accumulate(flow, mask, self.R, None if first else self.t, self.sums, _lib.EPI_T, self.scale_px,
                                       self.vote_px, self.blocks)
                    lib.epi_solve(self.sums, init_t, self.R, self.t, self.stats, H, W, _lib.EPI_T, self.gap_min, self.min_parallax_px)
                    first = False
        return self.R, self.t

    def estimate_bidirectional(self, r: BidirectionalFlow):
        """``estimate`` on what a bidirectional ``FlowStream`` returned: its forward flow, with the pixels of its forward occlusion
        mask (when the stream computes one) left out."""
        if not isinstance(r, BidirectionalFlow):
            raise PfError("PoseEstimator.estimate_bidirectional: r is what a bidirectional FlowStream returns")
        return self.estimate(r.forward, r.occ_forward)


def parallax_map(flow, R, t, mask=None, thr_px: float = 1.0, neg_px: float = 0.5, conf_min: float = 0.05, out=None, lib=None):
    """(inv_depth, resid, conf fp32 [B,H,W], moving uint8 [B,H,W]) of flow fp32 [B,2,H,W] under R [B,3,3] and t [B,3] (what
    ``PoseEstimator.estimate`` returned).  conf = |q x t|^2 is how far the pixel is from the epipoles (0 there, 1 on their
    equator); inv_depth = |T| / depth by triangulation on the sphere; resid is the pixel's distance from its epipolar great circle
    in pixel widths (360 degrees / W); moving = 1 where resid > thr_px or the parallax points away from the epipole by more than
    neg_px (a negative depth).  A left-out pixel (mask, or a flow that is not finite), a pixel with conf < conf_min and t = 0
    (an invalid fit) give inv_depth = 0, resid = 0, moving = 0.  thr_px = 1.0, neg_px = 0.5 and conf_min = 0.05 are choices, not
    measurements.  out: the four tensors to write (default: new ones)."""
    if not isinstance(flow, torch.Tensor) or flow.dim() != 4:
        raise PfError("parallax_map: flow must be a tensor [B,2,H,W]")
    lib = _library(flow.device, lib)
    B, _, H, W = flow.shape
    dev = flow.device
    _fit(flow, (B, 2, H, W), "parallax_map: flow", dev)
    _fit(R, (B, 3, 3), "parallax_map: R", dev)
    _fit(t, (B, 3), "parallax_map: t", dev)
    if mask is not None:
        _fit(mask, (B, H, W), "parallax_map: mask", dev, torch.uint8)
    if out is None:
        out = tuple(torch.empty(B, H, W, dtype=torch.float32, device=dev) for _ in range(3)) \
            + (torch.empty(B, H, W, dtype=torch.uint8, device=dev),)
    else:
        out = tuple(out)
        if len(out) != 4:
            raise PfError("parallax_map: out is (inv_depth, resid, conf, moving)")
        for o, what in zip(out[:3], ("inv_depth", "resid", "conf")):
            _fit(o, (B, H, W), f"parallax_map: {what}", dev)
        _fit(out[3], (B, H, W), "parallax_map: moving", dev, torch.uint8)
    with _on(dev):
        lib.epi_map(flow, mask, R, t, out[0], out[1], out[2], out[3], thr_px, neg_px, conf_min)
    return out
