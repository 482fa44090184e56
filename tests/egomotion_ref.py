"""Float64 numpy statement of the camera-rotation estimate, the tracker and the two appliers, written from
the definition and not from the kernel.  Not collected; imported by tests/test_egomotion_host.py and tests/test_hip_egomotion.py.

p = s(x, y), q = s(x + u, clamp(y + v, -1/2, H - 1/2)) with viewport_ref.sphere; a pixel is left out when its mask byte is
non-zero, its flow is not finite or |u| or |v| >= 2^30.  Pass k weighs it with cos phi(y) g_k, g_0 = 1 and
g_k = 1 / (1 + r^2 / c^2)^2 of the chord r = |q - R_{k-1} p|, c = scale_px 2 pi / W.  S = sum w p q^T, Horn's 4 x 4 matrix N,
the unit eigenvector of its largest eigenvalue with a >= 0, R its matrix.  The sums are kept between the calls the way the
library keeps them (the solve zeroes them), so that a pass that finds leftovers shows.

Every function takes `fault`: None, or the name of one deliberate mistake (FAULTS) that tests/test_egomotion_host.py builds into a
copy of the statement to show that the cases notice it.

The bounds (U = 2^-24, one fp32 rounding of a value below 1):
  BEARING = 64 U: the length of the error of a bearing evaluated in fp32.  theta = (((m + 1/2) / W - 1/2) 2) pi has four rounded
    steps on values of at most 2 W, 2, 3/2 and 2 pi and the sum x + u one more: d theta <= 8 pi U; phi the same on half the range:
    d phi <= 4 pi U; sinf and cosf are held to 2 ulp (2 U below 1), a product adds U: a component is off by at most
    d theta + d phi + 5 U, the vector by 3/2 of that = (18 pi + 7.5) U <= 64 U.
  rotation_bound(gap) = 48 BEARING / gap + 8 U, an ANGLE: with every p and q off by BEARING an entry of S = sum w p q^T moves by
    at most 2 BEARING sum w, an entry of N by three times that, |dN|_F <= 4 * 3 * 2 BEARING sum w; the unit eigenvector turns by at
    most |dN| / (lambda_1 - lambda_2) = 24 BEARING / gap (gap is per unit of weight), the rotation by twice that; the nine roundings
    of R and the quantisation of the sums (2^-32 of a weight and less) stay below 8 U.
  chord_bound = 176 U for a derotated flow, as a chord on the sphere: BEARING for q, 6 U for the product with R^T, 12 pi U for the
    two atan2f (8 U |angle| each), 14 pi U for the arithmetic of (m, n) (5 U W columns, 4 U H rows), and 3 pi U for a flow that was
    rounded to fp32 before it went in: (64 + 6 + 29 pi) U <= 176 U.
  position_budget: the same steps for the sample position of pf_erp_rotate, in pixels (towards a pole the column is ill-defined
    and the bound says so: 1 / rho).
"""
import numpy as np

import viewport_ref as vr

FAULTS = ("r_transposed", "no_cos_weight", "row_not_clamped", "no_reweight", "s_transposed", "quat_sign", "sums_not_zeroed",
          "u_not_wrapped")
U = 2.0 ** -24
BEARING = 64 * U
CHORD = 176 * U
FAR = 2.0 ** 30


def rotation_bound(gap):
    return 48 * BEARING / gap + 8 * U


def axis_angle(axis, deg):
    """Rodrigues: the rotation by deg degrees about axis, float64."""
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    a = np.radians(deg)
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


def yaw(cols, W):
    a = 2 * np.pi * cols / W
    return np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])


def angle_between(Ra, Rb):
    """The angle of Ra Rb^T, from its skew part and its trace (the arc cosine of the trace alone loses half the digits near 0)."""
    M = np.asarray(Ra, np.float64) @ np.asarray(Rb, np.float64).T
    sin = 0.5 * np.sqrt((M[2, 1] - M[1, 2]) ** 2 + (M[0, 2] - M[2, 0]) ** 2 + (M[1, 0] - M[0, 1]) ** 2)
    return float(np.arctan2(sin, (np.trace(M) - 1) / 2))


def grid(H, W):
    n, m = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    return m, n


def flow_of(R, H, W):
    """The flow [2,H,W] (float64) of the rigid rotation R: pixel (x, y) goes to erp(R s(x, y)), u in [-W/2, W/2)."""
    m, n = grid(H, W)
    qm, qn = vr.erp_of(vr.sphere(m, n, H, W) @ np.asarray(R, np.float64).T, H, W)
    return np.stack([np.mod(qm - m + W / 2, W) - W / 2, qn - n])


def left_out(flow, mask=None):
    """[B,H,W] bool."""
    with np.errstate(invalid="ignore"):
        out = ~(np.abs(flow[:, 0]) < FAR) | ~(np.abs(flow[:, 1]) < FAR)
    return out if mask is None else out | (np.asarray(mask) != 0)


def bearings(flow, fault=None):
    """(p [H,W,3], q [B,H,W,3]) of a flow [B,2,H,W]; entries that are not finite are read as 0 (the caller leaves them out)."""
    flow = np.nan_to_num(np.asarray(flow, np.float64), nan=0.0, posinf=0.0, neginf=0.0)
    B, _, H, W = flow.shape
    m, n = grid(H, W)
    en = n + flow[:, 1]
    if fault != "row_not_clamped":
        en = np.clip(en, -0.5, H - 0.5)
    return vr.sphere(m, n, H, W), vr.sphere(m + flow[:, 0], en, H, W)


def quat_canon(q, fault=None):
    q = np.asarray(q, np.float64)
    q = q / np.linalg.norm(q)
    return -q if (q[0] < 0 and fault != "quat_sign") else q


def quat_matrix(q):
    a, b, c, d = q
    return np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                     [2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)],
                     [2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d]])


def quat_of(R):
    """The unit quaternion of the rotation nearest to R (its polar factor), scalar part first, sign free."""
    u, _, vt = np.linalg.svd(np.asarray(R, np.float64))
    Q = u @ np.diag([1, 1, np.linalg.det(u @ vt)]) @ vt
    K = np.array([[Q[0, 0] + Q[1, 1] + Q[2, 2], Q[2, 1] - Q[1, 2], Q[0, 2] - Q[2, 0], Q[1, 0] - Q[0, 1]],
                  [0, Q[0, 0] - Q[1, 1] - Q[2, 2], Q[0, 1] + Q[1, 0], Q[0, 2] + Q[2, 0]],
                  [0, 0, -Q[0, 0] + Q[1, 1] - Q[2, 2], Q[1, 2] + Q[2, 1]],
                  [0, 0, 0, -Q[0, 0] - Q[1, 1] + Q[2, 2]]])
    K = K + np.triu(K, 1).T
    return np.linalg.eigh(K)[1][:, -1]


def quat_mul(x, y):
    a, b, c, d = x
    e, f, g, h = y
    return np.array([a * e - b * f - c * g - d * h, a * f + b * e + c * h - d * g, a * g - b * h + c * e + d * f,
                     a * h + b * g - c * f + d * e])


def slerp(x, y, t):
    if t <= 0:
        return x
    if t >= 1:
        return y
    dot = float(x @ y)
    if dot < 0:
        dot, y = -dot, -y
    if dot >= 1 - 1e-12:
        o = (1 - t) * x + t * y
    else:
        th = np.arccos(dot)
        o = (np.sin((1 - t) * th) * x + np.sin(t * th) * y) / np.sin(th)
    return o / np.linalg.norm(o)


class Estimator:
    """The estimate of one geometry with the library's state: twelve sums per image that a solve reads and zeroes."""

    def __init__(self, B, H, W, passes=4, scale_px=1.0, gap_min=1e-3, fault=None):
        self.B, self.H, self.W, self.passes, self.scale_px, self.gap_min, self.fault = B, H, W, passes, scale_px, gap_min, fault
        self.S = np.zeros((B, 3, 3))
        self.sw = np.zeros(B)
        self.swr = np.zeros(B)
        self.used = np.zeros(B)

    def accumulate(self, flow, mask, R, weighted):
        H, W, fault = self.H, self.W, self.fault
        p, q = bearings(flow, fault)
        out = left_out(np.asarray(flow), mask)
        phi = (0.5 - (np.arange(H) + 0.5) / H) * np.pi
        cosphi = np.broadcast_to(np.cos(phi)[:, None], (H, W))
        c = self.scale_px * 2 * np.pi / W
        for b in range(self.B):
            r2 = np.minimum(((q[b] - p @ np.asarray(R[b], np.float64).T) ** 2).sum(-1), 4.0)
            w = np.ones((H, W)) if fault == "no_cos_weight" else cosphi.copy()
            if weighted and fault != "no_reweight":
                w = w / (1 + r2 / c ** 2) ** 2
            w = np.where(out[b], 0.0, w)
            S = np.einsum("hw,hwa,hwb->ab", w, p, q[b])
            self.S[b] += S.T if fault == "s_transposed" else S
            self.sw[b] += w.sum()
            self.swr[b] += (w * r2).sum()
            self.used[b] += (~out[b]).sum()

    def solve(self, init):
        R, stats = np.zeros((self.B, 3, 3)), np.zeros((self.B, 5))
        for b in range(self.B):
            S, sw = self.S[b], self.sw[b]
            N = np.array([[S[0, 0] + S[1, 1] + S[2, 2], S[1, 2] - S[2, 1], S[2, 0] - S[0, 2], S[0, 1] - S[1, 0]],
                          [0, S[0, 0] - S[1, 1] - S[2, 2], S[0, 1] + S[1, 0], S[2, 0] + S[0, 2]],
                          [0, 0, -S[0, 0] + S[1, 1] - S[2, 2], S[1, 2] + S[2, 1]],
                          [0, 0, 0, -S[0, 0] - S[1, 1] + S[2, 2]]])
            N = N + np.triu(N, 1).T
            lam, vec = np.linalg.eigh(N)
            gap = (lam[-1] - lam[-2]) / sw if sw > 0 else 0.0
            valid = sw > 0 and gap >= self.gap_min
            R[b] = quat_matrix(quat_canon(vec[:, -1], self.fault)) if valid else init[b]
            if valid and self.fault == "r_transposed":
                R[b] = R[b].T
            stats[b] = [sw, np.sqrt(self.swr[b] / sw) if sw > 0 else 0.0, self.used[b] / (self.H * self.W), gap, float(valid)]
        if self.fault != "sums_not_zeroed":
            self.S[:], self.sw[:], self.swr[:], self.used[:] = 0, 0, 0, 0
        return R, stats

    def estimate(self, flow, mask=None, init=None, every_pass=False):
        """(R [B,3,3], stats [B,5]) of the last pass, or the list of every pass's."""
        init = np.broadcast_to(np.eye(3), (self.B, 3, 3)).copy() if init is None else np.asarray(init, np.float64)
        R, hist = init, []
        for k in range(self.passes):
            self.accumulate(flow, mask, R, k > 0)
            R, stats = self.solve(init)
            hist.append((R, stats))
        return hist if every_pass else hist[-1]


class Tracker:
    """O_t = R_t O_{t-1}, S_t = slerp(S_{t-1}, O_t, 1 - smoothing), C_t = O_t S_t^T; the state as the library holds it: two unit
    quaternions with a non-negative scalar part."""

    def __init__(self, smoothing, fault=None):
        self.t, self.fault = 1.0 - smoothing, fault
        self.o = np.array([1.0, 0, 0, 0])
        self.s = np.array([1.0, 0, 0, 0])

    def push(self, R):
        self.o = quat_canon(quat_mul(quat_canon(quat_of(R)), self.o), self.fault)
        self.s = quat_canon(slerp(self.s, self.o, self.t), self.fault)
        conj = self.s * np.array([1, -1, -1, -1.0])
        return quat_matrix(self.o), quat_matrix(quat_canon(quat_mul(self.o, conj)))


def rotate_positions(R, H, W):
    """(m, n, d) of every output pixel of pf_erp_rotate: the ERP position of d = R s(x, y)."""
    m, n = grid(H, W)
    d = vr.sphere(m, n, H, W) @ np.asarray(R, np.float64).T
    qm, qn = vr.erp_of(d, H, W)
    return qm, qn, d


def rotate(frame, R, fault=None):
    """[B,C,H,W] float64: frame sampled at erp(R s(x, y)), columns wrap, rows clamp."""
    frame = np.asarray(frame, np.float64)
    B, C, H, W = frame.shape
    out = np.zeros_like(frame)
    for b in range(B):
        Rb = np.asarray(R[b], np.float64)
        m, n, _ = rotate_positions(Rb.T if fault == "r_transposed" else Rb, H, W)
        ys, xs, ws, _ = vr.wraptaps(m, n, H, W)
        out[b] = (frame[b][:, ys, xs] * ws[None]).sum(1)
    return out


def rotate_u8(frame, R, fault=None):
    """uint8 [B,H,W,C] -> (the float64 value before rounding, floor(x + 1/2) clamped to 0..255), both [B,H,W,C]."""
    val = rotate(np.asarray(frame, np.float64).transpose(0, 3, 1, 2), R, fault).transpose(0, 2, 3, 1)
    return val, np.clip(np.floor(val + 0.5), 0, 255).astype(np.uint8)


def position_budget(R, H, W, extra=0.0):
    """(dm, dn) [H,W]: the fp32 budget of pf_erp_rotate's sample position in pixels, viewport_cases.position_budget's steps with
    the ray's budget dd = BEARING + 6 U (the bearing, then three products and two sums per component of R p) + extra (3 U when
    the comparison is with the exact rotation and not with the fp32 matrix that went in)."""
    _, _, d = rotate_positions(R, H, W)
    dd = BEARING + 6 * U + extra
    rho = np.hypot(d[..., 0], d[..., 1])
    theta, phi = np.arctan2(d[..., 1], d[..., 0]), np.arctan2(d[..., 2], rho)
    with np.errstate(divide="ignore"):
        dtheta = np.sqrt(2) * dd / rho + 8 * U * np.abs(theta)
    dphi = (dd * rho + (np.sqrt(2) * dd + 2 * U * rho) * np.abs(d[..., 2])) + 8 * U * np.abs(phi)
    return W * dtheta / (2 * np.pi) + 5 * U * W, H * dphi / np.pi + 4 * U * H


def value_bound(frame, R, extra=0.0):
    """[B,C,H,W]: (position budget) x (the largest difference of neighbouring pixels of the frame, per channel and direction)
    + the eight roundings of the four-tap mix.  The bilinear surface is Lipschitz with those differences across cell borders,
    the wrapped seam and the clamped pole rows included."""
    frame = np.asarray(frame, np.float64)
    B, C, H, W = frame.shape
    gx = np.abs(np.roll(frame, -1, 3) - frame).max((2, 3))                # [B,C]
    gy = np.abs(frame[:, :, 1:] - frame[:, :, :-1]).max((2, 3)) if H > 1 else np.zeros((B, C))
    top = np.abs(frame).max((2, 3))
    out = np.zeros_like(frame)
    for b in range(B):
        dm, dn = position_budget(R[b], H, W, extra)
        out[b] = dm[None] * gx[b][:, None, None] + dn[None] * gy[b][:, None, None] + 8 * U * top[b][:, None, None]
    return out


def derotate(flow, R, mask=None, fault=None):
    """(flow' [B,2,H,W], valid uint8 [B,H,W]): erp(R^T q) - (x, y), u' wrapped into [-W/2, W/2); (0, 0) where left out."""
    flow = np.asarray(flow)
    B, _, H, W = flow.shape
    _, q = bearings(flow, fault)
    out = left_out(flow, mask)
    m, n = grid(H, W)
    res = np.zeros((B, 2, H, W))
    for b in range(B):
        Rb = np.asarray(R[b], np.float64)
        qm, qn = vr.erp_of(q[b] @ (Rb.T if fault == "r_transposed" else Rb), H, W)           # rows of q times R = R^T q
        du = qm - m
        if fault != "u_not_wrapped":
            du = np.mod(du + W / 2, W) - W / 2
        res[b] = np.where(out[b], 0.0, np.stack([du, qn - n]))
    return res, (~out).astype(np.uint8)
