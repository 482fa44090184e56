"""Restatement of prior-flow_amd/csrc/pf_reproject.h in numpy: the projection in float64 with the fp32 budget
of its steps, the z-tested splat as the SAME fp32 steps (no transcendental is evaluated there, so numpy's float32 arithmetic gives
the statement's bits), and the update in either precision.

Every function takes `fault`: None, or the name of one deliberate mistake (FAULTS) that tests/test_reproject_host.py builds into a
twin of the code to show that a named check catches it.

The budget of the projection, in units of U = 2^-24 (egomotion_ref's constants):
  p                      BEARING per component (section 19)
  r = R p                BEARING + 6 U (three products, two sums)                                            = ROTATED
  s = r + d T            per component one product (U |d T_k|) and one sum (U |s_k|): ds = ROTATED + 2 U (|d| |T|_inf + |s|_inf)
  (qx, qy) = erp(s)      atan2 does not see the length of s: egomotion_ref.position_budget's steps on s / n with dd = ds / n
  u, v                   four roundings at the size of W (the difference, the half turn, the modulo, the half turn back), two at H
  n, d' = d / n          |dn| <= sqrt(3) ds + 3 U n (squares, sums, the root), then the division: rel(d') <= 2 ds / n + 6 U
"""
import numpy as np

import egomotion_ref as er
import viewport_ref as vr

FAULTS = ("d_not_divided", "t_sign", "r_transposed", "no_ztest", "ztest_min", "bmin_ignored", "front_not_cleared",
          "weights_not_normalised", "segment_ignored", "decay_dropped")
U = er.U
FAR = 2.0 ** 30
DEFAULTS = dict(b_min=0.25, ztol_log2=0.25, w_max=8.0, cmin=0.5, n_min=1e-6, dmax=65536.0, vmax=255.0, tol_log2=0.5, decay=0.9)
UPDATE_U = 8 * U          # two products, a sum, the decay, the weight sum and the division of the weighted mean, relative


# ---- project ---------------------------------------------------------------------------------------------------------------------
def left_out(inv_depth, weight, mask=None):
    d, w = np.asarray(inv_depth, np.float64), np.asarray(weight, np.float64)
    with np.errstate(invalid="ignore"):
        out = ~(w > 0) | ~((d >= 0) & (d < FAR))
    return out if mask is None else out | (np.asarray(mask) != 0)


def project(inv_depth, weight, R, T, mask=None, n_min=1e-6, fault=None):
    """float64: (flow [B,2,H,W], d_new [B,H,W], valid uint8 [B,H,W], s [B,H,W,3], n [B,H,W])."""
    d = np.nan_to_num(np.asarray(inv_depth, np.float64), nan=0.0, posinf=0.0, neginf=0.0)
    B, H, W = d.shape
    m, n = er.grid(H, W)
    p = vr.sphere(m, n, H, W)
    out = left_out(inv_depth, weight, mask)
    flow, dn, S, L = np.zeros((B, 2, H, W)), np.zeros((B, H, W)), np.zeros((B, H, W, 3)), np.ones((B, H, W))
    for b in range(B):
        Rb, Tb = np.asarray(R[b], np.float64), np.asarray(T[b], np.float64)
        if fault == "r_transposed":
            Rb = Rb.T
        if fault == "t_sign":
            Tb = -Tb
        s = p @ Rb.T + d[b][..., None] * Tb
        ln = np.ones((H, W)) if not Tb.any() else np.linalg.norm(s, axis=-1)
        near = ~(ln >= n_min)
        qm, qn = vr.erp_of(np.where(near[..., None], 1.0, s), H, W)
        f = np.stack([np.mod(qm - m + W / 2, W) - W / 2, qn - n])
        if not Tb.any() and (Rb == np.eye(3)).all():
            f[:] = 0.0                                                    # the same camera: nothing moves, bit for bit
        bad = out[b] | near
        out[b] = bad
        flow[b] = np.where(bad, 0.0, f)
        dn[b] = np.where(bad, 0.0, d[b] if fault == "d_not_divided" else d[b] / np.where(near, 1.0, ln))
        S[b], L[b] = s, ln
    return flow, dn, (~out).astype(np.uint8), S, L


def project_bound(inv_depth, T, S, L):
    """(du, dv [B,H,W] in pixels, rel [B,H,W]: the relative bound of d') for the values project() returned."""
    d = np.abs(np.nan_to_num(np.asarray(inv_depth, np.float64), nan=0.0, posinf=0.0, neginf=0.0))
    B, H, W = d.shape
    du, dv, rel = np.zeros((B, H, W)), np.zeros((B, H, W)), np.zeros((B, H, W))
    for b in range(B):
        ln = np.maximum(L[b], 1e-30)
        ds = er.BEARING + 6 * U + 2 * U * (d[b] * np.abs(np.asarray(T[b], np.float64)).max() + np.abs(S[b]).max(-1))
        dd = ds / ln
        sh = S[b] / ln[..., None]
        rho = np.hypot(sh[..., 0], sh[..., 1])
        theta, phi = np.arctan2(sh[..., 1], sh[..., 0]), np.arctan2(sh[..., 2], rho)
        with np.errstate(divide="ignore", invalid="ignore"):
            dtheta = np.sqrt(2) * dd / rho + 8 * U * np.abs(theta)
        dphi = (dd * rho + (np.sqrt(2) * dd + 2 * U * rho) * np.abs(sh[..., 2])) + 8 * U * np.abs(phi)
        du[b] = W * dtheta / (2 * np.pi) + 5 * U * W + 4 * U * W
        dv[b] = H * dphi / np.pi + 4 * U * H + 2 * U * H
        rel[b] = 2 * dd + 6 * U
    return du, dv, rel


def wrap_diff(a, b, W):
    """a - b of two horizontal flows, modulo W into [-W/2, W/2): +-W/2 name one displacement."""
    return np.mod(a - b + W / 2, W) - W / 2


# ---- the z-tested splat, in the statement's fp32 steps ------------------------------------------------------------------------
def scales(H, W, vmax):
    n = H * W
    lg = 0
    while (1 << lg) < n:
        lg += 1
    lv = 0
    while 2.0 ** lv < vmax:
        lv += 1
    return 62 - lg, 62 - lg - lv, lv


def _quant(v, s):
    """llrintf(v * 2^s) of float32 values (the product is exact: a power of two, no overflow for the values of a call)."""
    return np.rint(v.astype(np.float32) * np.float32(2.0 ** s)).astype(np.int64)


def zsplat(src, flow, d, weight, valid, front=None, acc=None, fault=None, **opt):
    """(front uint32 [B,H,W] before the resolve, acc int64 [B,C+3,H,W] before it, out [B,C,H,W] or None, d_out, w_out, hole,
    front after, acc after).  front / acc: what the buffers held before the call (default: zeros)."""
    o = dict(DEFAULTS, **opt)
    f32 = np.float32
    flow, d, weight = np.asarray(flow, f32), np.asarray(d, f32), np.asarray(weight, f32)
    B, H, W = d.shape
    C = 0 if src is None else src.shape[1]
    src = None if src is None else np.asarray(src, f32)
    N = H * W
    sd, sn, lv = scales(H, W, max(o["dmax"], o["vmax"]))
    front = np.zeros((B, H, W), np.uint32) if front is None else front.copy()
    acc = np.zeros((B, C + 3, H, W), np.int64) if acc is None else acc.copy()
    ztol = f32(np.exp2(np.float64(f32(o["ztol_log2"]))))           # exp2f, correctly rounded
    b_min = f32(0.0) if fault == "bmin_ignored" else f32(o["b_min"])
    w_max, dmax, vmax = f32(o["w_max"]), f32(o["dmax"]), f32(o["vmax"])
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    taps_of = []
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            qx, qy = xs.astype(f32) + flow[b, 0], ys.astype(f32) + flow[b, 1]
            ok = (valid[b] != 0) & (weight[b] > 0) & (d[b] >= 0) & (d[b] < f32(FAR)) & (np.abs(qx) < f32(FAR)) & (np.abs(qy) < f32(FAR))
            for c in range(C):
                ok &= np.abs(src[b, c]) < f32(FAR)
            qx, qy = np.where(ok, qx, f32(0)), np.where(ok, qy, f32(0))
            x0f, y0f = np.floor(qx), np.floor(qy)
            fx, fy = qx - x0f, qy - y0f
            gx, gy = f32(1) - fx, f32(1) - fy
            x0 = np.mod(x0f.astype(np.int64), W)
            x1 = np.where(x0 + 1 == W, 0, x0 + 1)
            y0 = y0f.astype(np.int64)
            dd = np.where(d[b] == 0, f32(0), d[b])
            wn = np.minimum(weight[b], w_max) if fault == "weights_not_normalised" else np.minimum(weight[b], w_max) / w_max
            taps = []
            for yy, xx, bk in ((y0, x0, gx * gy), (y0, x1, fx * gy), (y0 + 1, x0, gx * fy), (y0 + 1, x1, fx * fy)):
                use = ok & (yy >= 0) & (yy < H) & (bk >= b_min)
                if fault == "bmin_ignored":
                    use &= bk > 0
                taps.append((np.clip(yy, 0, H - 1)[use] * W + xx[use], bk[use], use))
            taps_of.append((taps, dd, wn))
            fr = front[b].reshape(-1)
            for idx, bk, use in taps:
                if fault == "ztest_min":
                    cur = np.where(fr == 0, np.uint32(0xFFFFFFFF), fr)
                    np.minimum.at(cur, idx, dd[use].view(np.uint32))
                    fr[:] = np.where(cur == np.uint32(0xFFFFFFFF), 0, cur)
                else:
                    np.maximum.at(fr, idx, dd[use].view(np.uint32))
        for b in range(B):
            taps, dd, wn = taps_of[b]
            fr = front[b].reshape(-1).view(f32)
            a = acc[b].reshape(C + 3, N)
            for idx, bk, use in taps:
                du = dd[use]
                if fault == "no_ztest":
                    cnt = np.ones(idx.shape, bool)
                elif fault == "ztest_min":
                    cnt = du <= fr[idx] * ztol
                else:
                    cnt = du * ztol >= fr[idx]
                idx, bk, du = idx[cnt], bk[cnt], du[cnt]
                wb = wn[use][cnt] * bk
                for c in range(C):
                    np.add.at(a[c], idx, _quant(wb * np.clip(src[b, c][use][cnt], -vmax, vmax), sn))
                np.add.at(a[C], idx, _quant(wb * np.minimum(du, dmax), sn))
                np.add.at(a[C + 1], idx, _quant(wb, sd))
                np.add.at(a[C + 2], idx, _quant(bk, sd))
    mid_front, mid_acc = front.copy(), acc.copy()
    D, cov = acc[:, C + 1].astype(np.float64), acc[:, C + 2].astype(np.float64)
    hole = ~(cov * 2.0 ** -sd >= np.float64(f32(o["cmin"]))) | (acc[:, C + 1] <= 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        val = lambda n: np.where(hole, 0.0, (n.astype(np.float64) / D) * 2.0 ** lv).astype(f32)          # noqa: E731
        out = None if C == 0 else np.stack([val(acc[:, c]) for c in range(C)], 1)
        d_out = val(acc[:, C])
        w_out = np.where(hole, 0.0, np.float64(w_max) * (D / cov)).astype(f32)
    after_front = front.copy() if fault == "front_not_cleared" else np.zeros_like(front)
    return mid_front, mid_acc, out, d_out, w_out, hole.astype(np.uint8), after_front, np.zeros_like(acc)


# ---- update ------------------------------------------------------------------------------------------------------------------
def update(d_s, w_s, d_m, w_m, disagree, flags, seg, dtype=np.float64, fault=None, **opt):
    """(d, w [B,H,W] of `dtype`, seg' int32 [B], decided [B,H,W] bool: a log2 was compared with tol there).  dtype float32 follows
    the statement step by step; its log2 is numpy's, which may differ from log2f in the last place."""
    o = dict(DEFAULTS, **opt)
    t = dtype
    ds, ws, dm, wm = (np.asarray(x, np.float32).astype(t) for x in (d_s, w_s, d_m, w_m))
    flags, seg = np.asarray(flags), np.asarray(seg)
    tol, decay, w_max = t(np.float32(o["tol_log2"])), t(np.float32(o["decay"])), t(np.float32(o["w_max"]))
    if fault == "decay_dropped":
        decay = t(1)
    same = (flags[:, 1] == seg)[:, None, None] | (fault == "segment_ignored")
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        counts = lambda d, w: (w > 0) & np.isfinite(w) & (d >= 0) & (d < t(FAR))                      # noqa: E731
        cs = same & counts(ds, ws)
        cm = counts(dm, wm) & ((np.asarray(disagree) == 0) if disagree is not None else True)
        wsc, wmc = np.minimum(ws, w_max), np.minimum(wm, w_max)
        near = np.abs(np.log2(dm / ds)) <= tol
        wd = decay * wsc
        tot = wd + wmc
        both = cs & cm
        d = np.where(both & near, (wd * ds + wmc * dm) / tot, np.where(both, dm, np.where(cs, ds, np.where(cm, dm, t(0)))))
        w = np.where(both & near, np.minimum(tot, w_max), np.where(both, wmc, np.where(cs, wd, np.where(cm, wmc, t(0)))))
        d, w = np.where(cs | cm, d, t(0)).astype(t), np.where(cs | cm, w, t(0)).astype(t)
    return d, w, flags[:, 1].astype(np.int32).copy(), both


def near_tol(d_s, d_m, tol, margin=64 * U):
    """[B,H,W] bool: |log2(d_m / d_s)| lies within `margin` of tol, so fp32 may decide the other way than float64."""
    with np.errstate(invalid="ignore", divide="ignore"):
        l = np.abs(np.log2(np.asarray(d_m, np.float64) / np.asarray(d_s, np.float64)))
    return np.abs(l - tol) <= margin


# ---- analytic scenes -------------------------------------------------------------------------------------------------------------
class Scene:
    """The inside of a sphere of radius `radius` about the origin (convex: nothing is ever occluded), optionally with a small sphere
    (centre, radius) in front of it.  A camera is (A, c): X_cam = A (X_world - c)."""

    def __init__(self, radius=4.0, ball=None):
        self.radius, self.ball = float(radius), ball

    def depth(self, A, c, H, W, ball=True, at=None):
        """(depth, on_ball bool, depth of the ball's FAR side or nan) along the bearings of the camera's ERP grid, or of the ERP
        positions at = (m, n) of any one shape."""
        m, n = er.grid(H, W) if at is None else at
        w = vr.sphere(m, n, H, W) @ np.asarray(A, np.float64)               # rows p^T A = (A^T p)^T
        c = np.asarray(c, np.float64)
        cw = w @ c
        rho = -cw + np.sqrt(cw * cw + self.radius ** 2 - c @ c)
        on, far = np.zeros(rho.shape, bool), np.full(rho.shape, np.nan)
        if ball and self.ball is not None:
            mc = np.asarray(self.ball[0], np.float64) - c
            mw = w @ mc
            disc = mw * mw - mc @ mc + self.ball[1] ** 2
            with np.errstate(invalid="ignore"):
                near, back = mw - np.sqrt(disc), mw + np.sqrt(disc)
            on = (disc >= 0) & (near > 0)
            rho, far = np.where(on, near, rho), np.where(on, back, np.nan)
        return rho, on, far


def relative_pose(cam0, cam1):
    """(R, T) with X_1 = R X_0 + T for two cameras (A, c)."""
    (A0, c0), (A1, c1) = cam0, cam1
    A0, A1 = np.asarray(A0, np.float64), np.asarray(A1, np.float64)
    return A1 @ A0.T, A1 @ (np.asarray(c0, np.float64) - np.asarray(c1, np.float64))


def reproject(src, inv_depth, weight, R, T, mask=None, fault=None, **opt):
    """The restatement of Reprojector.run: project in float64, stored as fp32, then the fp32 splat -> zsplat()'s tuple."""
    o = dict(DEFAULTS, **opt)
    flow, dn, valid, _, _ = project(inv_depth, weight, R, T, mask, o["n_min"], fault)
    return zsplat(src, flow.astype(np.float32), dn.astype(np.float32), weight, valid, fault=fault, **opt)
