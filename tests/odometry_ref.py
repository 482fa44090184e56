"""Float64 numpy statement of the scale link, the pose chain and the fused depth, written from the definition
and not from the kernel.  Not collected; imported by tests/test_odometry_host.py and tests/test_hip_odometry.py.  The scenes, the
pose estimate and the parallax map are epipolar_ref's.

A MAP is (kappa, conf, moving) on one grid.  Link pixel: left out when a moving byte is set, !(conf > 0) or !(kappa_min <= kappa <
2^30) for either map; else w = cos phi min(conf_a, 1) min(conf_b, 1), l = log2(kappa_b / kappa_a), l_c = clip(l, -L, L), bin =
clip(floor((l_c + L) bins / (2 L)), 0, bins - 1).  Histogram W[bin] += w, M[bin] += w l_c / L.  Solve: the median bin m is the
smallest with 2 C >= total (C the inclusive prefix sum), q1, q3 likewise with 4 C >= total, 4 C >= 3 total; l^ = L sum M / sum W
over [m - trim, m + trim] cut to the range; ratio = 2^l^; valid = 0 (ratio 1) when total = 0, used < min_used, iqr > max_iqr or m is
a clamp bin.

Every function takes `fault`: None, or the name of one deliberate mistake (FAULTS) that tests/test_odometry_host.py builds into a
copy of the statement to show that the cases notice it.

The bounds (U = 2^-24), each for ONE launch given the same fp32 inputs:
  edge_rounding(L): how far the fp32 l of the code may lie from the float64 l, in units of l, by the time it is binned.  The
    division kappa_b / kappa_a is off by U relative, which log2 turns into U / ln 2 absolute; log2f itself by at most 2 ulp of its
    result, 4 U L at the most; l_c + L by U 2 L; the product with bins and the division by 2 L by U relative each of a value
    whose l-equivalent is at most 2 L: together (1 / ln 2 + 4 L + 3 * 2 L) U = (1 / ln 2 + 10 L) U.  A pixel whose float64 l lies
    within that of a bin edge may land in either bin; every other pixel must land in the restatement's bin.
  W_ABS = 8 U, W_REL = 4 U: the weight.  phi(y) of a row is a handful of fp32 operations on values below pi / 2 and cosf is good
    to an ulp, so cos phi is off by at most 8 U absolute (NOT relative: it is small near the poles); the two products and the
    fp32 values of min(conf, 1) add 2 U relative, the quantisation at 2^S (S >= 32 for every shape here) less than U.
  lhat_bound(...): l^ is a weighted mean of l over a window of width (2 trim + 1) bins.  Moving a share f of the window's weight
    in or out of the window, or rescaling weights by a relative eps, moves the mean by at most (f + 2 eps) times that width; each l
    itself is off by edge_rounding, and M's own two operations by 2 U L.
  Track: every step is a handful of fp64 operations on fp32 inputs and an fp32 store: 8 U per step on values of size <= 1, scaled
    by the size of the value (the centre grows with the path).
  Fuse: d = kappa / S, two products, a sum and a division: 5 U relative of the larger d (a convex combination), with the weight
    sum off by U.  disagree: log2f(d_b / d_a) is off by (3 / ln 2 + 4 tol) U near the threshold.
"""
import numpy as np

import egomotion_ref as er
import epipolar_ref as pr

FAULTS = ("no_cos_weight", "moving_ignored", "ratio_inverted", "mean_over_all_bins", "clamp_bins_valid", "window_not_cut",
          "scale_before_validity", "b_not_rotated", "fuse_wrong_scale")
U = er.U
FAR = 2.0 ** 30
W_ABS, W_REL = 8 * U, 4 * U
STATS = 6
DEFAULTS = dict(bins=512, log2_range=4.0, trim_bins=4, kappa_min=1e-4, min_used=0.05, max_iqr=1.0)


def edge_rounding(L):
    return (1 / np.log(2) + 10 * L) * U


def cos_rows(H):
    return np.cos((0.5 - (np.arange(H) + 0.5) / H) * np.pi)


# ---- link ------------------------------------------------------------------------------------------------------------------------
def link_terms(map_a, map_b, bins=512, log2_range=4.0, kappa_min=1e-4, fault=None, rows=None):
    """dict of [B,H,W] float64 arrays: used (bool), w, l (unclamped), lc, bin (int), near (bool: l within edge_rounding of a bin
    edge).  rows: cos phi per row (default: float64)."""
    ka, ca, ma = (np.asarray(x) for x in map_a)
    kb, cb, mb = (np.asarray(x) for x in map_b)
    B, H, W = ka.shape
    L = float(log2_range)
    kmin = np.float32(kappa_min)
    with np.errstate(invalid="ignore"):
        ok = (ca > 0) & (cb > 0) & (ka >= kmin) & (ka < FAR) & (kb >= kmin) & (kb < FAR)
    if fault != "moving_ignored":
        ok &= (ma == 0) & (mb == 0)
    ka64, kb64 = np.where(ok, ka, 1.0).astype(np.float64), np.where(ok, kb, 1.0).astype(np.float64)
    cosphi = np.ones(H) if fault == "no_cos_weight" else (cos_rows(H) if rows is None else np.asarray(rows, np.float64))
    w = cosphi[None, :, None] * np.minimum(np.where(ok, ca, 0.0).astype(np.float64), 1.0) * np.minimum(np.where(ok, cb, 0.0).astype(np.float64), 1.0)
    l = np.log2(ka64 / kb64) if fault == "ratio_inverted" else np.log2(kb64 / ka64)
    lc = np.clip(l, -L, L)
    pos = (lc + L) * bins / (2 * L)
    b = np.clip(np.floor(pos), 0, bins - 1).astype(np.int64)
    near = np.abs(pos - np.round(pos)) * (2 * L / bins) <= edge_rounding(L)
    near &= (np.round(pos) > 0) & (np.round(pos) < bins)                 # the ends of the range are no edges: the clamp takes both sides
    return dict(used=ok, w=np.where(ok, w, 0.0), l=l, lc=lc, bin=b, near=near & ok)


def histogram(k, bins, L):
    """(W [B,bins], M [B,bins], total [B], count [B]) in float64 from link_terms' dict."""
    B = k["w"].shape[0]
    Wh, Mh = np.zeros((B, bins)), np.zeros((B, bins))
    for b in range(B):
        u = k["used"][b]
        Wh[b] = np.bincount(k["bin"][b][u], weights=k["w"][b][u], minlength=bins)
        Mh[b] = np.bincount(k["bin"][b][u], weights=(k["w"][b] * k["lc"][b] / L)[u], minlength=bins)
    return Wh, Mh, k["w"].sum((1, 2)), k["used"].sum((1, 2))


def first_at_least(C, thr):
    return int(np.searchsorted(C, thr, side="left"))


def solve(Wh, Mh, total, count, HW, bins=512, log2_range=4.0, trim_bins=4, min_used=0.05, max_iqr=1.0, fault=None):
    """(ratio [B], stats [B,6], info: list of dict(m, q1, q3, lo, hi)) from float64 or integer histograms."""
    B = Wh.shape[0]
    L = float(log2_range)
    ratio, stats, info = np.ones(B), np.zeros((B, STATS)), []
    for b in range(B):
        # integer histograms (the code's cells) are compared as Python integers: 4 C does not fit 64 bits
        cells = [int(v) for v in Wh[b]] if np.issubdtype(Wh.dtype, np.integer) else [float(v) for v in Wh[b]]
        tot = sum(cells)
        m = q1 = q3 = lo = hi = 0
        lhat = share = 0.0
        if tot > 0:
            C = np.cumsum(np.array(cells, dtype=object))
            m, q1, q3 = (next(i for i, c in enumerate(C) if k * c >= n * tot) for k, n in ((2, 1), (4, 1), (4, 3)))
            if fault == "window_not_cut":
                idx = np.arange(m - trim_bins, m + trim_bins + 1) % bins
            else:
                lo, hi = max(m - trim_bins, 0), min(m + trim_bins, bins - 1)
                idx = np.arange(lo, hi + 1)
            if fault == "mean_over_all_bins":
                idx = np.arange(bins)
            ws, ms = float(Wh[b][idx].sum()), float(Mh[b][idx].sum())
            lhat, share = L * ms / ws, ws / float(tot)
        used = count[b] / HW
        iqr = (q3 - q1) * 2 * L / bins
        clamp = m in (0, bins - 1) and fault != "clamp_bins_valid"
        valid = tot > 0 and used >= np.float32(min_used) and iqr <= np.float32(max_iqr) and not clamp
        ratio[b] = 2.0 ** lhat if valid else 1.0
        stats[b] = [float(total[b]), used, lhat, iqr, share, float(valid)]
        info.append(dict(m=m, q1=q1, q3=q3, lo=lo, hi=hi))
    return ratio, stats, info


def link(map_a, map_b, fault=None, rows=None, **opt):
    """(ratio [B], stats [B,6], detail) of two maps: detail = dict(terms, W, M, info)."""
    o = dict(DEFAULTS, **opt)
    k = link_terms(map_a, map_b, o["bins"], o["log2_range"], o["kappa_min"], fault, rows)
    Wh, Mh, total, count = histogram(k, o["bins"], o["log2_range"])
    H, W = k["w"].shape[1:]
    ratio, stats, info = solve(Wh, Mh, total, count, H * W, o["bins"], o["log2_range"], o["trim_bins"], o["min_used"], o["max_iqr"], fault)
    return ratio, stats, dict(terms=k, W=Wh, M=Mh, info=info, total=total, count=count)


def lhat_bound(detail, b, bins, L, trim):
    """The distance by which the code's l^ of image b may differ from the restatement's, and the share of near pixels (by weight,
    of the window's weight) behind it."""
    k, inf = detail["terms"], detail["info"][b]
    lo, hi = max(inf["lo"] - 1, 0), min(inf["hi"] + 1, bins - 1)
    inwin = (k["bin"][b] >= lo) & (k["bin"][b] <= hi) & k["used"][b]
    wwin = detail["W"][b][inf["lo"]:inf["hi"] + 1].sum()
    near_w = k["w"][b][inwin & k["near"][b]].sum()
    eps = (W_ABS * inwin.sum() + W_REL * k["w"][b][inwin].sum()) / wwin
    width = (2 * trim + 1) * 2 * L / bins
    return edge_rounding(L) + 2 * U * L + (near_w / wwin + 2 * eps) * width, near_w / wwin


# ---- reverse pose, track -----------------------------------------------------------------------------------------------------------
def reverse_pose(R, t):
    R, t = np.asarray(R, np.float64), np.asarray(t, np.float64)
    Rt = R.transpose(0, 2, 1)
    return Rt, -np.einsum("bij,bj->bi", Rt, t)


class Track:
    """The chain of B videos: A [B,3,3], b [B,3], S, steps, segment, prev_valid, all float64."""

    def __init__(self, B, fault=None):
        self.B, self.fault = B, fault
        self.reset()

    def reset(self):
        B = self.B
        self.A, self.b, self.S = np.stack([np.eye(3)] * B), np.zeros((B, 3)), np.ones(B)
        self.steps, self.segment, self.prev = np.zeros(B, int), np.zeros(B, int), np.zeros(B, bool)

    def step(self, R, t, pose_valid, ratio, link_valid):
        """-> (orientation [B,3,3], centre [B,3], baseline [B], flags [B,4])"""
        R, t = np.asarray(R, np.float64), np.asarray(t, np.float64)
        flags = np.zeros((self.B, 4), int)
        for i in range(self.B):
            pv, lv = bool(pose_valid[i]), bool(link_valid[i])
            self.A[i] = R[i] @ self.A[i]
            if self.fault != "b_not_rotated":
                self.b[i] = R[i] @ self.b[i]
            if self.fault == "scale_before_validity":
                self.S[i] *= ratio[i]
            if pv:
                if self.prev[i] and lv:
                    if self.fault != "scale_before_validity":
                        self.S[i] *= ratio[i]
                else:
                    self.segment[i] += 1
                self.b[i] = self.b[i] + self.S[i] * t[i]
            self.prev[i] = pv
            self.steps[i] += 1
            flags[i] = [self.steps[i], self.segment[i], pv, lv]
        centre = -np.einsum("bji,bj->bi", self.A, self.b)
        return self.A.copy(), centre, self.S.copy(), flags


# ---- fuse ------------------------------------------------------------------------------------------------------------------------
def fuse_edge(tol):
    return (3 / np.log(2) + 4 * tol) * U


def fuse(map_a, map_b, S_a, S_b, link_valid, conf_min=0.05, kappa_min=1e-4, tol_log2=0.5, fault=None):
    """(inv_depth, weight float64 [B,H,W], disagree uint8, near [B,H,W] bool: |log2(d_b / d_a)| within fuse_edge of the threshold,
    scale [B,H,W]: the larger of the two d, which the element's rounding is relative to)."""
    ka, ca, ma = (np.asarray(x) for x in map_a)
    kb, cb, mb = (np.asarray(x) for x in map_b)
    S_a, S_b = np.asarray(S_a, np.float64)[:, None, None], np.asarray(S_b, np.float64)[:, None, None]
    if fault == "fuse_wrong_scale":
        S_a, S_b = S_b, S_a
    cm = np.float32(conf_min)
    with np.errstate(invalid="ignore"):
        oka = (ma == 0) & (ca >= cm) & (ka >= 0) & (ka < FAR) & (np.asarray(link_valid)[:, None, None] != 0)
        okb = (mb == 0) & (cb >= cm) & (kb >= 0) & (kb < FAR)
    wa, wb = np.where(oka, ca, 0.0).astype(np.float64), np.where(okb, cb, 0.0).astype(np.float64)
    da, db = np.where(oka, ka, 0.0) / S_a, np.where(okb, kb, 0.0) / S_b
    ws = wa + wb
    with np.errstate(invalid="ignore", divide="ignore"):
        some = (ws > 0) & np.isfinite(ws)                             # a weight sum of 0 or inf counts nothing
        inv = np.where(some, (wa * da + wb * db) / np.where(some, ws, 1.0), 0.0)
        ws = np.where(some, ws, 0.0)
        both = oka & okb & (ka >= np.float32(kappa_min)) & (kb >= np.float32(kappa_min))
        dl = np.abs(np.log2(np.where(both, db, 1.0) / np.where(both, da, 1.0)))
    dis = both & (dl > np.float32(tol_log2))
    near = both & (np.abs(dl - np.float32(tol_log2)) <= fuse_edge(tol_log2))
    return inv, ws, dis.astype(np.uint8), near, np.maximum(da, db)
