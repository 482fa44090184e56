"""Float64 numpy statement of the camera-translation estimate and the parallax map, written from the
definition and not from the kernel.  Not collected; imported by tests/test_epipolar_host.py and tests/test_hip_epipolar.py.  The
bearings, the left-out rule and the rotation estimate are egomotion_ref's, the sphere viewport_ref's.

Model: q ~ R p + kappa t, t a unit vector, kappa = |T| / depth >= 0 (a POINT of the scene moves by T in the second frame's axes;
the camera centre moves along -R^T t in the first frame's).  Per pixel, with r = R p:
  n = r x q,  vote n^ = n / sqrt(|n|^2 + c_v^2), c_v = vote_px 2 pi / W
  m = t x r,  e = (q . m) / |m| when |m|^2 >= 1e-12, else 0,  e^2 clamped to 1
  w = cos phi / (1 + e^2 / c^2)^2, c = scale_px 2 pi / W
  d = (q - r) - ((q - r) . r) r
  e_a = t . n,  g = (t . r) q - (r . q) t
T pass: M = sum w n^ n^T, D = sum w d, sum w, sum w e^2, sum w |n|^2, count; t = the eigenvector of M's smallest eigenvalue, turned
so that t . D >= 0.  R pass: G = sum w g g^T, h = sum w e_a g, dw = -G^-1 h, R <- exp([dw]x) R.  The sums are kept between the calls
the way the library keeps them (a solve zeroes what it read), so that a pass that finds leftovers shows.

Every function takes `fault`: None, or the name of one deliberate mistake (FAULTS) that tests/test_epipolar_host.py builds into a
copy of the statement to show that the cases notice it.

The bounds (U = 2^-24; BEARING = 64 U is egomotion_ref's: the length of the error of a bearing evaluated in fp32).  Every bound is
for ONE launch given the same fp32 inputs (flow, R, t): the tests walk the schedule launch by launch and give the restatement the
state the code under test left behind, so that no bound inherits the slack of the one before (a chain of worst cases over eight
passes says nothing: the iteration contracts, the worst cases multiply).
  ROTATED = BEARING + 6 U: r = R p in fp32 (the bearing, three products and two sums per component).
  NORMAL = 160 U >= ROTATED + BEARING + 9 U: n = r x q with both off (|r|, |q| <= 1), six products and three differences; the
    same budget holds e = q . m / |m| wherever |m| is not tiny, and e_a = t . n.
  t_pass_bound: a vote n^ = n / sqrt(|n|^2 + c_v^2) has |d n^| <= |dn| / c_v, so |dM|_F <= 3 * 2 (NORMAL / c_v) sum w from the
    votes.  A weight moves by |dg| <= (1.3 / c) NORMAL (g's steepest slope, at e = c / sqrt 5), but what that does to the
    eigenvector goes through M's action on t, sum dw n^ (n^ . t) with |n^ . t| = |e| |m| / sqrt(|n|^2 + c_v^2) <= |e| / c_v: at
    most 1.3 NORMAL e_rms / (c c_v) sum w, nothing on a scene without residuals.  The unit eigenvector turns by at most twice
    |dM t| / (lambda_2 - lambda_1) (Davis-Kahan), lambda_2 - lambda_1 = gap * trace M; the fp32 store of t and the quantisation
    of the sums (2^-32 of a weight and less) stay below 8 U.
      bound = 2 (6 NORMAL / c_v + 1.3 NORMAL e_rms / (c c_v)) (sum w / trace M) / gap + 8 U          (an ANGLE)
  r_pass_bound: dw = -G^-1 h.  g_w is off by DG = 288 U (two products of a dot product off by ROTATED + BEARING + 3 U with a unit
    vector), h = sum w e_a g_w by (NORMAL |g_w| + |e_a| DG) sum w <= (2 NORMAL + DG) sum w, G by 4 DG sum w:
      bound = (2 NORMAL + DG + 4 DG |dw|) sum w / lambda_min(G) + 8 U                                 (an ANGLE)
  kappa, resid per pixel (given the same R and t): kappa = (n . (q x t)) / |q x t|^2 has the numerator off by NORMAL + 2 BEARING
    |n| and the denominator relatively by 4 BEARING / |q x t|: 4 NORMAL (1 + |kappa|) / |q x t| covers both; resid = |e| W / 2 pi
    with e off by 2 NORMAL / |t x r|, and |t x r| >= |q x t| - |n|.
"""
import numpy as np

import egomotion_ref as er

FAULTS = ("no_cos_weight", "no_vote_norm", "no_reweight", "no_sign", "r_transposed", "dw_right", "kappa_swapped",
          "row_not_clamped", "sums_not_zeroed")
U = er.U
BEARING = er.BEARING
ROTATED = BEARING + 6 * U
NORMAL = 160 * U
STATS = 6


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def angle_vec(a, b):
    """The angle between two vectors, from the cross and the dot product."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.arctan2(np.linalg.norm(np.cross(a, b)), a @ b))


def px(angle, W):
    """An angle in pixel widths (360 degrees / W)."""
    return angle * W / (2 * np.pi)


# ---- scenes ----------------------------------------------------------------------------------------------------------------------
def depth_smooth(H, W):
    m, n = er.grid(H, W)
    return 3 + 1.5 * np.sin(6 * np.pi * m / W) * np.cos(2 * np.pi * n / H) + 0.8 * np.cos(10 * np.pi * m / W + 1)


def depth_room(H, W):
    """A floor 1.6 below the camera, its slope capped at 0.2 (which puts the walls at 8)."""
    m, n = er.grid(H, W)
    pz = er.vr.sphere(m, n, H, W)[..., 2]
    return 1.6 / np.maximum(-pz, 0.2)


DEPTHS = {"smooth": depth_smooth, "room": depth_room}


def scene_flow(R, t, T, rho):
    """The flow [2,H,W] (float64) of the static scene rho p under x -> R x + T t: the exact projection, u in [-W/2, W/2)."""
    H, W = rho.shape
    m, n = er.grid(H, W)
    X = (rho[..., None] * er.vr.sphere(m, n, H, W)) @ np.asarray(R, np.float64).T + T * unit(t)
    qm, qn = er.vr.erp_of(X, H, W)
    return np.stack([np.mod(qm - m + W / 2, W) - W / 2, qn - n])


def moved_block(H, W):
    """[H,W] bool: rows H/4..H/2, columns W/8..W/8 + 0.3 W (7.5 % of the pixels)."""
    blk = np.zeros((H, W), bool)
    blk[H // 4:H // 2, W // 8:W // 8 + int(0.3 * W)] = True
    return blk


# ---- the per-pixel quantities ------------------------------------------------------------------------------------------------------
def _cross(a, b):
    return np.cross(a, b)


def pixel_terms(flow, R, t, scale_px, fault=None):
    """Everything a pass needs of image-batch flow [B,2,H,W] under R [B,3,3], t [B,3]: dict of [B,H,W(,3)] arrays."""
    flow = np.asarray(flow)
    B, _, H, W = flow.shape
    p, q = er.bearings(flow, fault)
    R = np.asarray(R, np.float64)
    t = np.asarray(t, np.float64)
    if fault == "r_transposed":
        R = R.transpose(0, 2, 1)
    r = np.einsum("bij,hwj->bhwi", R, p)
    tb = t[:, None, None, :]
    n = _cross(r, q)
    m = _cross(np.broadcast_to(tb, r.shape), r)
    mm = (m * m).sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(mm >= 1e-12, (q * m).sum(-1) / np.sqrt(mm), 0.0)
    e2 = np.minimum(e * e, 1.0)
    c = scale_px * 2 * np.pi / W
    g = np.ones_like(e2) if fault == "no_reweight" else 1 / (1 + e2 / c ** 2) ** 2
    phi = (0.5 - (np.arange(H) + 0.5) / H) * np.pi
    cosphi = np.ones((H, W)) if fault == "no_cos_weight" else np.broadcast_to(np.cos(phi)[:, None], (H, W))
    return dict(p=p, q=q, r=r, n=n, m=m, mm=mm, e=e, e2=e2, w=cosphi[None] * g, tb=tb)


class Pose:
    """The estimate of one geometry with the library's state: the 22 sums per image, which a solve reads and zeroes."""

    def __init__(self, B, H, W, t_passes=4, rounds=2, scale_px=1.0, vote_px=0.25, gap_min=1e-3, min_parallax_px=0.05, fault=None,
                 **rotation):
        self.B, self.H, self.W, self.t_passes, self.rounds = B, H, W, t_passes, rounds
        self.scale_px, self.vote_px, self.gap_min, self.min_parallax_px, self.fault = scale_px, vote_px, gap_min, min_parallax_px, fault
        self.rot = er.Estimator(B, H, W, **rotation)
        self.M, self.D, self.G, self.h = np.zeros((B, 3, 3)), np.zeros((B, 3)), np.zeros((B, 3, 3)), np.zeros((B, 3))
        self.sw, self.swe, self.swn, self.used = np.zeros(B), np.zeros(B), np.zeros(B), np.zeros(B)

    def accumulate(self, mode, flow, mask, R, t):
        k = pixel_terms(flow, R, t, self.scale_px, self.fault)
        out = er.left_out(np.asarray(flow), mask)
        w = np.where(out, 0.0, k["w"])
        q, r, n = k["q"], k["r"], k["n"]
        self.sw += w.sum((1, 2))
        self.used += (~out).sum((1, 2))
        if mode == 0:
            nn = (n * n).sum(-1)
            cv = self.vote_px * 2 * np.pi / self.W
            nh = n if self.fault == "no_vote_norm" else n / np.sqrt(nn + cv ** 2)[..., None]
            d = (q - r) - ((q - r) * r).sum(-1, keepdims=True) * r
            self.M += np.einsum("bhw,bhwi,bhwj->bij", w, nh, nh)
            self.D += np.einsum("bhw,bhwi->bi", w, d)
            self.swe += (w * k["e2"]).sum((1, 2))
            self.swn += (w * nn).sum((1, 2))
        else:
            ea = (k["tb"] * n).sum(-1)
            g = (k["tb"] * r).sum(-1, keepdims=True) * q - (r * q).sum(-1, keepdims=True) * k["tb"]
            self.G += np.einsum("bhw,bhwi,bhwj->bij", w, g, g)
            self.h += np.einsum("bhw,bhw,bhwi->bi", w, ea, g)

    def _zero(self, *names):
        if self.fault != "sums_not_zeroed":
            for nm in names:
                getattr(self, nm)[...] = 0

    def solve_t(self, t_init):
        t, stats = np.zeros((self.B, 3)), np.zeros((self.B, STATS))
        self.last_t = np.zeros(self.B)                              # trace M / sum w, for t_pass_bound
        k = self.W / (2 * np.pi)
        for b in range(self.B):
            sw = self.sw[b]
            lam, vec = np.linalg.eigh(self.M[b])
            tr = lam.sum()
            gap = (lam[1] - lam[0]) / tr if (sw > 0 and tr > 0) else 0.0
            par = k * np.sqrt(self.swn[b] / sw) if sw > 0 else 0.0
            valid = sw > 0 and gap >= self.gap_min and par >= self.min_parallax_px
            v = vec[:, 0]
            if v @ self.D[b] < 0 and self.fault != "no_sign":
                v = -v
            t[b] = v if valid else (t_init[b] if t_init is not None else 0.0)
            stats[b] = [sw, k * np.sqrt(self.swe[b] / sw) if sw > 0 else 0.0, self.used[b] / (self.H * self.W), gap, par, float(valid)]
            self.last_t[b] = tr / sw if sw > 0 else 0.0
        self._zero("M", "D", "sw", "swe", "swn", "used")
        return t, stats

    def solve_r(self, R, t, stats):
        out = np.array(R, np.float64)
        self.last_r = np.zeros((self.B, 2))                         # lambda_min(G) / sum w and |dw|, for r_pass_bound
        for b in range(self.B):
            lam, vec = np.linalg.eigh(self.G[b])
            self.last_r[b, 0] = lam[0] / self.sw[b] if self.sw[b] > 0 else 0.0
            if stats[b, 5] and (t[b] != 0).any() and lam.sum() > 0 and lam[0] >= 1e-9 * lam.sum():
                dw = -vec @ ((vec.T @ self.h[b]) / lam)
                self.last_r[b, 1] = np.linalg.norm(dw)
                E = er.axis_angle(dw, np.degrees(np.linalg.norm(dw))) if np.linalg.norm(dw) > 0 else np.eye(3)
                out[b] = out[b] @ E if self.fault == "dw_right" else E @ out[b]
        self._zero("G", "h", "sw", "used")
        return out

    def schedule(self):
        """The launches of an estimate after the rotation estimate: ("T" | "R", first) per pass."""
        out = []
        for rnd in range(self.rounds):
            if rnd:
                out.append(("R", False))
            out += [("T", rnd == 0 and i == 0) for i in range(self.t_passes)]
        return out

    def step(self, kind, first, flow, mask, R, t, stats, init_t=None):
        """One pass (an accumulate and its solve) from the state (R, t, stats) -> the state after it."""
        if kind == "R":
            self.accumulate(1, flow, mask, R, t)
            return self.solve_r(R, t, stats), t, stats
        self.accumulate(0, flow, mask, R, np.zeros((self.B, 3)) if first else t)
        t, stats = self.solve_t(init_t)
        return np.array(R, np.float64), t, stats

    def estimate(self, flow, mask=None, init_R=None, init_t=None, history=False):
        """(R [B,3,3], t [B,3], stats [B,6], R0 = the rotation-only answer); history: also the list of (R, t, stats) after every
        pass."""
        R0, _ = self.rot.estimate(flow, mask, init_R)
        R, t, stats = np.array(R0), np.zeros((self.B, 3)), np.zeros((self.B, STATS))
        hist = []
        for kind, first in self.schedule():
            R, t, stats = self.step(kind, first, flow, mask, R, t, stats, init_t)
            hist.append((R.copy(), t.copy(), stats.copy()))
        return (R, t, stats, R0, hist) if history else (R, t, stats, R0)


def parallax(flow, R, t, mask=None, thr_px=1.0, neg_px=0.5, conf_min=0.05, fault=None):
    """(inv_depth, resid, conf [B,H,W] float64, moving [B,H,W] uint8, a [B,H,W]: the signed parallax behind `moving`)."""
    flow = np.asarray(flow)
    W = flow.shape[3]
    k = pixel_terms(flow, R, t, 1.0, fault)
    out = er.left_out(flow, mask)
    q, n = k["q"], k["n"]
    qt = _cross(q, np.broadcast_to(k["tb"], q.shape))
    conf = np.where(out, 0.0, (qt * qt).sum(-1))
    ok = ~out & (conf >= conf_min) & (conf > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        nv = -n if fault == "kappa_swapped" else n
        a = np.where(ok, (nv * qt).sum(-1) / np.sqrt(conf), 0.0)
        kappa = np.where(ok, a / np.sqrt(conf), 0.0)
    resid = np.where(ok, np.abs(k["e"]) * W / (2 * np.pi), 0.0)
    moving = ok & ((resid > thr_px) | (a < -neg_px * 2 * np.pi / W))
    return kappa, resid, conf, moving.astype(np.uint8), a


# ---- bounds ------------------------------------------------------------------------------------------------------------------------
DG = 288 * U


def t_pass_bound(stats, trace_sw, W, vote_px=0.25, scale_px=1.0):
    """The angle by which the t of ONE T pass may differ from the restatement's on the same inputs; stats: the restatement's row,
    trace_sw: trace M / sum w of that pass (Pose.last_t)."""
    cv, c = vote_px * 2 * np.pi / W, scale_px * 2 * np.pi / W
    e_rms = stats[1] * 2 * np.pi / W
    return 2 * (6 * NORMAL / cv + 1.3 * NORMAL * e_rms / (c * cv)) / (trace_sw * stats[3]) + 8 * U


def r_pass_bound(lmin_sw, dw):
    """The angle by which the R of ONE R pass may differ; lmin_sw: lambda_min(G) / sum w, dw: |dw| (Pose.last_r)."""
    return (2 * NORMAL + DG + 4 * DG * dw) / lmin_sw + 8 * U
