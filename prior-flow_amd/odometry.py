"""Camera trajectory from 360-degree video on the device: the scale link between consecutive pairs, the pose chain and depth
fused in one unit.

    stream = FlowStream(model, iters=12, bidirectional=True, occlusion="sphere")
    odo = Odometry(B, H, W, device)
    for frame in frames:
        r = stream(frame)
        if r is not None:
            orientation, centre = odo.push(r)               # the camera of the LATER frame in the first frame's axes
            odo.inv_depth, odo.depth_weight, odo.disagree   # of the pair's EARLIER frame, in trajectory units

``PoseEstimator`` (section 20) gives every pair a unit translation and a depth map "up to the baseline".  What links one pair to
the next is the frame they share: the backward flow of pair k and the forward flow of pair k + 1 both live on its grid, so
``parallax_map`` on the first (under the reversed pose) gives kappa_a = |T_k| / rho and on the second kappa_b = |T_k+1| / rho with
the SAME depth rho, and kappa_b / kappa_a is the ratio of the two baselines at every static pixel.  ``ScaleLink`` takes a robust
location of log2 of that ratio over the frame: a weighted histogram in 64-bit integers (the same bits on every run), its median
bin, and the weighted mean of the bins around it.  The unit of the trajectory is the baseline of the first pair of a segment;
metric scale is not observable.  There is no CPU path: tensors on the host are refused (PfError).
"""
from __future__ import annotations

import math

import torch

from . import _lib
from ._lib import PfError
from .egomotion import _device, _fit, _library, _on
from .parallax import PoseEstimator, parallax_map
from .video import BidirectionalFlow


def _fit_map(m, B, H, W, what, dev):
    if not isinstance(m, (tuple, list)) or len(m) != 3:
        raise PfError(f"{what} is (inv_depth, conf, moving), the first, third and fourth tensor of parallax_map")
    _fit(m[0], (B, H, W), f"{what}: inv_depth", dev)
    _fit(m[1], (B, H, W), f"{what}: conf", dev)
    _fit(m[2], (B, H, W), f"{what}: moving", dev, torch.uint8)
    return tuple(m)


class ScaleLink:
    """The ratio |T_b| / |T_a| of the baselines behind two parallax maps of ONE grid, every buffer allocated here.

    A pixel counts when neither map calls it moving, both conf > 0 and both kappa lie in [kappa_min, 2^30); its weight is its solid
    angle times min(conf, 1) of both maps, its value l = log2(kappa_b / kappa_a) clamped to +-log2_range.  The histogram has
    ``bins`` bins over that range; the answer is 2^(weighted mean of l over the median bin +- trim_bins).  ``stats`` [B,6] = {sum
    of weights, used fraction, l^, interquartile range of l (in bins, as log2), weight of the window / total, valid}.  valid = 0
    (and ratio = 1) when nothing counted, fewer than min_used of the pixels counted, the interquartile range exceeds max_iqr or
    the median fell into the first or last bin, where the clamped values collect.

    bins = 512, log2_range = 4, trim_bins = 4, kappa_min = 1e-4, min_used = 0.05 and max_iqr = 1.0 are choices, not measurements
    (DESIGN.md section 22 says what they were tried on)."""

    def __init__(self, B: int, H: int, W: int, device, bins: int = 512, log2_range: float = 4.0, trim_bins: int = 4,
                 kappa_min: float = 1e-4, min_used: float = 0.05, max_iqr: float = 1.0, lib=None, blocks: int = 0):
        self.lib = _library(device, lib)
        self.device = _device(device)
        if int(bins) != bins or bins < 64 or bins > 1024 or bins & (bins - 1):
            raise PfError(f"ScaleLink: bins = {bins!r}, expected a power of two in 64..1024")
        if int(trim_bins) != trim_bins or trim_bins < 0 or trim_bins > bins:
            raise PfError(f"ScaleLink: trim_bins = {trim_bins!r}, expected an integer in 0..bins")
        if not all(math.isfinite(v) for v in (log2_range, kappa_min, min_used, max_iqr)) \
                or not (0 < log2_range <= 64 and kappa_min > 0 and min_used >= 0 and max_iqr > 0):
            raise PfError(f"ScaleLink: log2_range {log2_range!r}, kappa_min {kappa_min!r}, min_used {min_used!r}, max_iqr {max_iqr!r}")
        self.B, self.H, self.W, self.blocks = B, H, W, int(blocks)
        self.bins, self.log2_range, self.trim_bins = int(bins), float(log2_range), int(trim_bins)
        self.kappa_min, self.min_used, self.max_iqr = float(kappa_min), float(min_used), float(max_iqr)
        self.lib.odo_hist_bytes(B, H, W, self.bins)                # the geometry the library accepts
        self.hist = torch.zeros(B, 2 * self.bins + 2, dtype=torch.int64, device=self.device)
        self.ratio = torch.ones(B, dtype=torch.float32, device=self.device)
        self.stats = torch.zeros(B, _lib.ODO_STATS, dtype=torch.float32, device=self.device)

    def link(self, map_a, map_b):
        """(ratio [B], stats [B,6]) (``self.ratio``, ``self.stats``, overwritten by the next call): one accumulate and one solve.
        A map is (inv_depth, conf, moving) of ``parallax_map``."""
        B, H, W, dev = self.B, self.H, self.W, self.device
        map_a, map_b = _fit_map(map_a, B, H, W, "ScaleLink.link: map_a", dev), _fit_map(map_b, B, H, W, "ScaleLink.link: map_b", dev)
        with _on(dev):
            self.hist.zero_()                                     # all-zero after every completed call; a cut-short one costs nothing
            self.lib.odo_accumulate(map_a, map_b, self.hist, self.bins, self.log2_range, self.kappa_min, self.blocks)
            self.lib.odo_solve(self.hist, self.ratio, self.stats, H, W, self.bins, self.log2_range, self.trim_bins, self.min_used,
                               self.max_iqr)
        return self.ratio, self.stats


def fuse_depth(map_a, map_b, S_a, S_b, link_valid, conf_min: float = 0.05, kappa_min: float = 1e-4, tol_log2: float = 0.5, out=None,
               lib=None):
    """(inv_depth, weight fp32 [B,H,W], disagree uint8 [B,H,W]) of two parallax maps (inv_depth, conf, moving) of one grid whose
    baselines are the device scalars S_a, S_b [B]: d = kappa / S, averaged with the maps' conf as weights.  A map counts at a
    pixel where it is not moving, conf >= conf_min and 0 <= kappa < 2^30; map a only where link_valid [B] is non-zero.  disagree = 1
    where both count, both kappa >= kappa_min and the two d differ by more than a factor 2^tol_log2.  conf_min = 0.05, kappa_min =
    1e-4 and tol_log2 = 0.5 are choices, not measurements.  out: the three tensors to write (default: new ones)."""
    if not isinstance(map_a, (tuple, list)) or len(map_a) != 3 or not isinstance(map_a[0], torch.Tensor) or map_a[0].dim() != 3:
        raise PfError("fuse_depth: map_a is (inv_depth, conf, moving) with tensors [B,H,W]")
    dev = map_a[0].device
    lib = _library(dev, lib)
    B, H, W = map_a[0].shape
    map_a, map_b = _fit_map(map_a, B, H, W, "fuse_depth: map_a", dev), _fit_map(map_b, B, H, W, "fuse_depth: map_b", dev)
    if not all(math.isfinite(v) for v in (conf_min, kappa_min, tol_log2)) or not (conf_min >= 0 and kappa_min > 0 and tol_log2 > 0):
        raise PfError(f"fuse_depth: conf_min {conf_min!r}, kappa_min {kappa_min!r}, tol_log2 {tol_log2!r}")
    for x, what in ((S_a, "S_a"), (S_b, "S_b"), (link_valid, "link_valid")):
        _fit(x, (B,), f"fuse_depth: {what}", dev)
    if out is None:
        out = (torch.empty(B, H, W, dtype=torch.float32, device=dev), torch.empty(B, H, W, dtype=torch.float32, device=dev),
               torch.empty(B, H, W, dtype=torch.uint8, device=dev))
    else:
        out = tuple(out)
        if len(out) != 3:
            raise PfError("fuse_depth: out is (inv_depth, weight, disagree)")
        _fit(out[0], (B, H, W), "fuse_depth: inv_depth", dev)
        _fit(out[1], (B, H, W), "fuse_depth: weight", dev)
        _fit(out[2], (B, H, W), "fuse_depth: disagree", dev, torch.uint8)
    with _on(dev):
        lib.odo_fuse(map_a, map_b, S_a, S_b, link_valid, out[0], out[1], out[2], conf_min, kappa_min, tol_log2)
    return out


_POSE_KEYS = ("t_passes", "rounds", "scale_px", "vote_px", "gap_min", "min_parallax_px", "passes")
_LINK_KEYS = ("bins", "log2_range", "trim_bins", "kappa_min", "min_used", "max_iqr")
_MAP_KEYS = ("thr_px", "neg_px", "conf_min")
_STATE0 = (1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0)


class Odometry:
    """The camera path of B videos from what a bidirectional ``FlowStream`` returns, with every buffer allocated here.  It owns a
    ``PoseEstimator`` (``.pose``) and a ``ScaleLink`` (``.scale``); the options of both, ``parallax_map``'s thr_px / neg_px /
    conf_min and ``fuse_depth``'s tol_log2 are keyword arguments.

    ``push(r)`` runs on the current stream, reads nothing on the host, allocates nothing after the first push and can be captured
    into a HIP graph: the pose of the pair; map b of its forward flow; the link against map a of the pair before (the first push
    has none: ratio 1, link valid 0); the track step; the fused depth; the reversed pose and map a of the backward flow for the
    next push.  It returns (orientation [B,3,3], centre [B,3]) of the later frame's camera in the axes of the first frame, the
    centre in units of the baseline of the first pair of the current segment, and keeps ``baseline`` [B], ``flags`` int32 [B,4] =
    {steps, segment, pose valid, link valid}, ``ratio`` [B], ``link_stats`` [B,6] and ``inv_depth``, ``depth_weight``,
    ``disagree`` [B,H,W] of the pair's earlier frame.  A pair without an observable translation (pose valid = 0) turns the camera,
    leaves the centre where it was and starts a new segment."""

    def __init__(self, B: int, H: int, W: int, device, lib=None, blocks: int = 0, tol_log2: float = 0.5, **options):
        unknown = [k for k in options if k not in _POSE_KEYS + _LINK_KEYS + _MAP_KEYS]
        if unknown:
            raise PfError(f"Odometry: unknown options {unknown}")
        self.pose = PoseEstimator(B, H, W, device, lib=lib, blocks=blocks, **{k: v for k, v in options.items() if k in _POSE_KEYS})
        self.lib, self.device = self.pose.lib, self.pose.device
        self.scale = ScaleLink(B, H, W, self.device, lib=self.lib, blocks=blocks, **{k: v for k, v in options.items() if k in _LINK_KEYS})
        self.map_options = {k: float(v) for k, v in options.items() if k in _MAP_KEYS}
        self.tol_log2 = float(tol_log2)
        if not (self.tol_log2 > 0 and math.isfinite(self.tol_log2)):
            raise PfError(f"Odometry: tol_log2 = {tol_log2!r}")
        self.B, self.H, self.W = B, H, W
        dev = self.device
        f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)                    # noqa: E731
        u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8, device=dev)                       # noqa: E731
        # map = (inv_depth, resid, conf, moving) as parallax_map writes it
        self.map_a = (f32(B, H, W), f32(B, H, W), f32(B, H, W), u8(B, H, W))
        self.map_b = (f32(B, H, W), f32(B, H, W), f32(B, H, W), u8(B, H, W))
        self.R_rev, self.t_rev = f32(B, 3, 3), f32(B, 3)
        self.state0 = torch.tensor(_STATE0, dtype=torch.float64, device=dev).repeat(B, 1).contiguous()
        self.state = self.state0.clone()
        self.orientation, self.centre = f32(B, 3, 3), f32(B, 3)
        self.baseline, self.prev_baseline, self.link_valid = f32(B), f32(B), f32(B)
        self.flags = torch.zeros(B, _lib.ODO_FLAGS, dtype=torch.int32, device=dev)
        self.ratio, self.link_stats = self.scale.ratio, self.scale.stats
        self.inv_depth, self.depth_weight, self.disagree = f32(B, H, W), f32(B, H, W), u8(B, H, W)
        self.reset()

    def reset(self):
        """Forget the path: the next push is the first one.  Every buffer of the state is rewritten."""
        with _on(self.device):
            self.state.copy_(self.state0)
            self.baseline.fill_(1.0)
            self.prev_baseline.fill_(1.0)
            self.link_valid.zero_()
            self.flags.zero_()
            self.ratio.fill_(1.0)
            self.link_stats.zero_()
            self.scale.hist.zero_()
            for m in (self.map_a, self.map_b):
                for x in m:
                    x.zero_()                                       # an all-zero map a: conf = 0 leaves every pixel out
            self.R_rev.zero_()
            self.t_rev.zero_()
            self.orientation.copy_(self.pose.estimator.identity)
            self.centre.zero_()
            for x in (self.inv_depth, self.depth_weight, self.disagree):
                x.zero_()

    @staticmethod
    def _triple(m):
        return (m[0], m[2], m[3])

    def push_flows(self, forward, backward, occ_forward=None, occ_backward=None):
        """``push`` on the four tensors themselves: forward = flow(previous -> frame), backward = flow(frame -> previous) fp32
        [B,2,H,W], and their occlusion masks uint8 [B,H,W] or None."""
        B, H, W, dev, lib = self.B, self.H, self.W, self.device, self.lib
        _fit(backward, (B, 2, H, W), "Odometry.push: backward", dev)
        if occ_backward is not None:
            _fit(occ_backward, (B, H, W), "Odometry.push: occ_backward", dev, torch.uint8)
        R, t = self.pose.estimate(forward, occ_forward)             # checks forward and occ_forward
        with _on(dev):
            parallax_map(forward, R, t, mask=occ_forward, out=self.map_b, lib=lib, **self.map_options)
            a, b = self._triple(self.map_a), self._triple(self.map_b)
            # the first push links against the all-zero map a of reset(): nothing counts, ratio 1, valid 0
            self.scale.link(a, b)
            self.prev_baseline.copy_(self.baseline)
            lib.odo_track(R, t, self.pose.stats, self.ratio, self.link_stats, self.state, self.orientation, self.centre,
                          self.baseline, self.flags)
            self.link_valid.copy_(self.link_stats[:, 5])
            lib.odo_fuse(a, b, self.prev_baseline, self.baseline, self.link_valid, self.inv_depth, self.depth_weight, self.disagree,
                         self.map_options.get("conf_min", 0.05), self.scale.kappa_min, self.tol_log2)
            lib.odo_reverse_pose(R, t, self.R_rev, self.t_rev)
            parallax_map(backward, self.R_rev, self.t_rev, mask=occ_backward, out=self.map_a, lib=lib, **self.map_options)
        return self.orientation, self.centre

    def push(self, r: BidirectionalFlow):
        """One pair of the video: what a bidirectional ``FlowStream`` returned -> (orientation [B,3,3], centre [B,3])."""
        if not isinstance(r, BidirectionalFlow):
            raise PfError("Odometry.push: r is what a bidirectional FlowStream returns")
        return self.push_flows(r.forward, r.backward, r.occ_forward, r.occ_backward)
