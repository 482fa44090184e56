"""Float64 restatement of the forward-backward check (include/priorflow_hip.h: pf_fb_check), the
constructed flow fields its tests run on, and the bounds a result is held to.  Written from the statement, not from the kernel.

One direction: f = the flow on the grid of its first frame, g = the opposite flow.  At p = (x, y): q = p + f; g^ = g sampled
at q (x wrapped with Python's modulo, y clamped, bilinear weights from the unclamped fraction), the u of the three non-anchor
taps first brought to within W/2 of the anchor tap; r = (u_clip(f_u + g^_u), f_v + g^_v).
plane:  occluded <=> |r|^2 > alpha (|f|^2 + |g^|^2) + beta.
sphere: d = Haversine distance of ERP points, theta = ((x + 0.5) / W - 0.5) 2 pi, phi = (0.5 - (y + 0.5) / H) pi, the
        haversine clamped to [0, 1]; occluded <=> d(p, p + r)^2 > alpha (d(p, q)^2 + d(q, p + r)^2) + beta (2 pi / W)^2.

Bounds (each from the number format, none from a kernel's output):
  residual  tol(p) = 4 * 2^-23 * (W + |f_u| + |f_v| + |g^_u| + |g^_v|) * (1 + S),  S = spread of the four un-wrapped u taps +
            spread of the four v taps: q is an fp32 number of size W, off by up to 2^-23 W, and the bilinear blend turns a
            position error d into a value error d * S.  u is compared modulo W.
  mask      with L = sqrt(lhs), T = sqrt(rhs) (sphere: both in equatorial pixels) a pixel is DECIDED when
            |L - T| > 2 tol(p) + 1e-3 T; a decided pixel must carry the float64 decision; at most 1 % of a case's pixels
            may be undecided.
"""
import numpy as np

KINDS = ("smooth", "seam", "poles")
SEEDS = (3, 4)                      # image 0, image 1 of a batch
MAX_UNDECIDED = 0.01


def pair(kind: str, H: int, W: int, seed: int):
    """(forward, backward) flows [2,H,W] float32 of one image.  Draw order of default_rng(seed): the forward noise of u, of v,
    then the backward noise [2,H,W]."""
    g = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    if kind == "smooth":
        u = 6.0 * np.sin(2 * np.pi * x / W + 0.3) + 2.0
        v = 3.0 * np.cos(np.pi * y / H)
    elif kind == "seam":            # flows at the +-W/2 boundary, neighbouring rows 0.2 W apart
        u = np.where((y > 0.4 * H) & (y < 0.6 * H), W / 2 - 3.0, 0.3 * W) + 2.0 * np.sin(y / 7.0)
        v = 4.0 * np.sin(4 * np.pi * x / W)
    elif kind == "poles":           # rows leave the frame at the top and at the bottom
        u = 5.0 * np.cos(2 * np.pi * y / H)
        v = 0.3 * (y - H / 2)
    else:
        raise ValueError(kind)
    u = u + g.normal(0, 0.05, (H, W))
    v = v + g.normal(0, 0.05, (H, W))
    fw = np.stack([u, v]).astype(np.float32)
    # backward: -f scattered to the nearest pixel of p + f (x wrapped, y clamped; raster order, the last writer stays), zero
    # where nothing lands, noise, and a block that disagrees
    f64 = fw.astype(np.float64)
    tx = np.mod(np.rint(x + f64[0]), W).astype(np.int64) % W
    ty = np.clip(np.rint(y + f64[1]), 0, H - 1).astype(np.int64)
    bw = np.zeros((2, H, W))
    bw[0, ty.ravel(), tx.ravel()] = -f64[0].ravel()
    bw[1, ty.ravel(), tx.ravel()] = -f64[1].ravel()
    bw = bw + g.normal(0, 0.3, (2, H, W))
    bw[0, H // 4:H // 2, W // 8:W // 3] += 7.0
    bw[1, H // 4:H // 2, W // 8:W // 3] -= 5.0
    return fw, bw.astype(np.float32)


def batch(kind: str, H: int, W: int):
    """(forward, backward) [2,2,H,W] float32: image 0 from default_rng(3), image 1 from default_rng(4)."""
    ps = [pair(kind, H, W, s) for s in SEEDS]
    return np.stack([p[0] for p in ps]), np.stack([p[1] for p in ps])


def _haversine_dist(xa, ya, xb, yb, H, W):
    th = lambda x: ((x + 0.5) / W - 0.5) * 2 * np.pi        # noqa: E731
    ph = lambda y: (0.5 - (y + 0.5) / H) * np.pi            # noqa: E731
    hav = lambda t: np.sin(t / 2) ** 2                      # noqa: E731
    h = hav(ph(yb) - ph(ya)) + np.cos(ph(ya)) * np.cos(ph(yb)) * hav(th(xb) - th(xa))
    return 2 * np.arcsin(np.sqrt(np.clip(h, 0.0, 1.0)))


def reference(f32: np.ndarray, g32: np.ndarray, metric: str, alpha: float = 0.01, beta: float = 0.5) -> dict:
    """One image, one direction: f32, g32 [2,H,W] float32.  Returns float64 maps: r [2,H,W], occ (bool), L, T (pixels),
    tol, and `bad` (non-finite f or g^: occluded, r = 0)."""
    f, g = f32.astype(np.float64), g32.astype(np.float64)
    _, H, W = f.shape
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        qx, qy = x + f[0], y + f[1]
        gx = np.mod(qx, W)
        fx, fy = np.floor(gx), np.floor(qy)
        xw, yw = gx - fx, qy - fy
        ok = np.isfinite(fx) & np.isfinite(fy)
        x0 = np.where(ok, fx, 0).astype(np.int64) % W
        x1 = (x0 + 1) % W
        y0 = np.clip(np.where(ok, fy, 0), 0, H - 1).astype(np.int64)
        y1 = np.clip(np.where(ok, fy, 0) + 1, 0, H - 1).astype(np.int64)
        taps = ((y0, x0), (y1, x0), (y0, x1), (y1, x1))           # a (anchor), b, c, d
        wts = ((1 - xw) * (1 - yw), (1 - xw) * yw, xw * (1 - yw), xw * yw)
        us = [g[0][t] for t in taps]
        us = [us[0]] + [us[0] + np.mod(u - us[0] + W / 2, W) - W / 2 for u in us[1:]]
        vs = [g[1][t] for t in taps]
        gu = sum(w * u for w, u in zip(wts, us))
        gv = sum(w * v for w, v in zip(wts, vs))
        ru = np.mod(f[0] + gu + W / 2, W) - W / 2
        rv = f[1] + gv
        bad = ~(np.isfinite(f[0]) & np.isfinite(f[1]) & np.isfinite(gu) & np.isfinite(gv))
        S = (np.max(us, 0) - np.min(us, 0)) + (np.max(vs, 0) - np.min(vs, 0))
        tol = 4 * 2.0 ** -23 * (W + abs(f[0]) + abs(f[1]) + abs(gu) + abs(gv)) * (1 + S)
        if metric == "plane":
            L = np.sqrt(ru ** 2 + rv ** 2)
            T = np.sqrt(alpha * (f[0] ** 2 + f[1] ** 2 + gu ** 2 + gv ** 2) + beta)
        elif metric == "sphere":
            sr = _haversine_dist(x, y, x + ru, y + rv, H, W)
            sf = _haversine_dist(x, y, qx, qy, H, W)
            sg = _haversine_dist(qx, qy, x + ru, y + rv, H, W)
            px = 2 * np.pi / W
            L = sr / px
            T = np.sqrt(alpha * (sf ** 2 + sg ** 2) + beta * px ** 2) / px
        else:
            raise ValueError(metric)
    occ = (L > T) | bad
    r = np.stack([np.where(bad, 0.0, ru), np.where(bad, 0.0, rv)])
    return dict(r=r, occ=occ, L=L, T=T, tol=tol, bad=bad, W=W)


def check(occ: np.ndarray, res: np.ndarray, ref: dict, what="") -> dict:
    """occ [H,W] uint8 and res [2,H,W] float32 of one image and direction against `reference`'s answer.  Prints the figures,
    then asserts the bounds of the module docstring; returns the figures."""
    W, tol, bad = ref["W"], ref["tol"], ref["bad"]
    assert set(np.unique(occ)) <= {0, 1}, what
    du = np.mod(res[0].astype(np.float64) - ref["r"][0] + W / 2, W) - W / 2
    dv = res[1].astype(np.float64) - ref["r"][1]
    good = ~bad
    worst = float(max(np.max(np.abs(du[good]) / tol[good]), np.max(np.abs(dv[good]) / tol[good]))) if good.any() else 0.0
    with np.errstate(invalid="ignore"):
        decided = (np.abs(ref["L"] - ref["T"]) > 2 * tol + 1e-3 * ref["T"]) | bad
    wrong = int(((occ != 0) != ref["occ"])[decided].sum())
    figures = dict(residual_err_over_tol=worst, undecided=float(1 - decided.mean()), wrong_decided=wrong,
                   differ_undecided=int(((occ != 0) != ref["occ"])[~decided].sum()), occluded=float(ref["occ"].mean()))
    print(what, figures)
    assert worst <= 1.0, (what, figures)
    assert not res[:, bad].any() and occ[bad].all(), what
    assert figures["undecided"] <= MAX_UNDECIDED, (what, figures)
    assert wrong == 0, (what, figures)
    return figures
