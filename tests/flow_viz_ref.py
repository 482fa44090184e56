"""From-scratch float64 numpy restatement of the flow rendering, used where no fixture exists and pinned
against tests/golden/flow_viz.npz by tests/test_flow_viz_host.py.  Written from the formulas, not from the kernels:

  veclen_spherical(flow)       great-circle length of the flow: the Haversine distance (R = 1) between the pixel centre and its end
                               point (x wraps into [-0.5, W - 0.5), y clamps to [-0.5, H - 0.5]) under the ERP map
                               theta = ((x + 0.5) / W - 0.5) 2 pi, phi = (0.5 - (y + 0.5) / H) pi
  colorwheel()                 the 55-entry Middlebury wheel
  render(flow, mode, ...)      uint8 [B,H,W,3]: rad = min(len, clip) / (clip + 1e-5), a = atan2(-v, -u) / pi, blend of wheel entries
                               floor(fk) and floor(fk) + 1 at fk = (a + 1) / 2 * 54, col = 1 - rad (1 - blend), floor(255 col)
  cycle_warp(x, flo)           bilinear sample at the fp32 position (x + u, y + v): x wraps, y clamps, weights from the unclamped
                               fraction
"""
import numpy as np


def veclen_spherical(flow):
    f = np.asarray(flow, np.float64)
    B, _, H, W = f.shape
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ex = np.mod(xx + f[:, 0] + 0.5, W) - 0.5
    ey = np.clip(yy + f[:, 1], -0.5, H - 0.5)
    th = lambda x: ((x + 0.5) / W - 0.5) * 2 * np.pi      # noqa: E731
    ph = lambda y: (0.5 - (y + 0.5) / H) * np.pi          # noqa: E731
    hav = lambda t: np.sin(t / 2) ** 2                    # noqa: E731
    h = hav(ph(ey) - ph(yy)) + np.cos(ph(yy)) * np.cos(ph(ey)) * hav(th(ex) - th(xx))
    return 2 * np.arcsin(np.sqrt(np.clip(h, 0.0, 1.0)))


def colorwheel():
    segs = ((15, 0, 1, +1), (6, 1, 0, -1), (4, 1, 2, +1), (11, 2, 1, -1), (13, 2, 0, +1), (6, 0, 2, -1))   # n, full, ramp, direction
    rows = []
    for n, full, ramp, sign in segs:
        for i in range(n):
            c = [0.0, 0.0, 0.0]
            c[full] = 255.0
            r = np.floor(255.0 * i / n)
            c[ramp] = r if sign > 0 else 255.0 - r
            rows.append(c)
    return np.array(rows)


def lengths(flow, mode):
    f = np.asarray(flow, np.float64)
    ok = np.isfinite(f[:, 0]) & np.isfinite(f[:, 1])
    g = np.where(ok[:, None], f, 0.0)
    ln = veclen_spherical(g) if mode == "omni" else np.sqrt(g[:, 0] ** 2 + g[:, 1] ** 2)
    return np.where(ok, ln, np.nan)             # a pixel whose flow is not finite ranks last (numpy sorts NaN last)


def clip_values(length, mode, percentile=0.95):
    """Per image: sort(len)[int(percentile n)] (omni) or the maximum (plane); `length` in the precision it was computed in.  NaN
    (a flow that is not finite) sorts last; a rank that falls on one takes the largest value that is not NaN (none: 0)."""
    B = length.shape[0]
    n = length[0].size
    k = n - 1 if mode == "plane" else min(int(percentile * n), n - 1)
    out = []
    for b in range(B):
        s = np.sort(length[b], axis=None)
        good = s[~np.isnan(s)]
        out.append(s[k] if not np.isnan(s[k]) else (good[-1] if len(good) else 0.0))
    return np.array(out)


def render(flow, mode="omni", percentile=0.95, bgr=False, length=None, clip=None):
    """uint8 [B,H,W,3].  `length` / `clip` override the float64 ones (e.g. the fp32 values a kernel produced), so that the colour
    stage can be compared on its own."""
    f = np.asarray(flow, np.float64)
    ln = lengths(f, mode) if length is None else np.asarray(length, np.float64)
    cl = clip_values(ln, mode, percentile) if clip is None else np.asarray(clip, np.float64)
    wheel = colorwheel() / 255.0
    bad = ~(np.isfinite(f[:, 0]) & np.isfinite(f[:, 1]))
    f = np.where(bad[:, None], 0.0, f)
    rad = np.minimum(np.where(bad, 0.0, ln), cl[:, None, None]) / (cl[:, None, None] + 1e-5)
    a = np.arctan2(-f[:, 1], -f[:, 0]) / np.pi
    fk = (a + 1) / 2 * 54
    k0 = np.clip(np.floor(fk).astype(np.int64), 0, 54)
    k1 = np.where(k0 + 1 == 55, 0, k0 + 1)
    t = (fk - k0)[..., None]
    col = (1 - t) * wheel[k0] + t * wheel[k1]
    col = np.where(rad[..., None] <= 1, 1 - rad[..., None] * (1 - col), 0.75 * col)
    img = np.clip(np.floor(255 * col), 0, 255).astype(np.uint8)
    img[bad] = 0
    return img[..., ::-1].copy() if bgr else img


def cycle_warp(x, flo):
    x = np.asarray(x, np.float64)
    B, C, H, W = x.shape
    # the sample position is an fp32 tensor in the definition (grid + flo, then x % W: my_cycle_sample.py:108-111, :31): its
    # rounding belongs to the statement (one ulp of a position near 100 px moves a 0..255 image by up to 1e-3); everything after
    # it (fractions, weights, the blend) is float64
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    f = np.asarray(flo, np.float32)
    gx = np.mod(xx + f[:, 0], np.float32(W)).astype(np.float64)
    gy = (yy + f[:, 1]).astype(np.float64)
    fx, fy = np.floor(gx), np.floor(gy)
    wx, wy = (gx - fx)[:, None], (gy - fy)[:, None]
    x0 = fx.astype(np.int64) % W
    x1 = (x0 + 1) % W
    y0 = np.clip(fy.astype(np.int64), 0, H - 1)
    y1 = np.clip(fy.astype(np.int64) + 1, 0, H - 1)
    bi = np.arange(B)[:, None, None, None]
    ci = np.arange(C)[None, :, None, None]
    g = lambda y, xq: x[bi, ci, y[:, None], xq[:, None]]      # noqa: E731
    return (1 - wx) * (1 - wy) * g(y0, x0) + (1 - wx) * wy * g(y1, x0) + wx * (1 - wy) * g(y0, x1) + wx * wy * g(y1, x1)


def photometric(ref, warped, occ=None):
    """err [B,H,W] = mean over channels of |ref - warped|; mean_err [B] over occ == 0 (all pixels without a mask; none: 0)."""
    err = np.abs(np.asarray(ref, np.float64) - np.asarray(warped, np.float64)).mean(axis=1)
    keep = np.ones(err.shape, bool) if occ is None else (np.asarray(occ) == 0)
    cnt = keep.reshape(len(err), -1).sum(1)
    s = np.where(keep, err, 0.0).reshape(len(err), -1).sum(1)
    return err, np.where(cnt > 0, s / np.maximum(cnt, 1), 0.0)
