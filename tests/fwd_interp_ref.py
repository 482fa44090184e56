"""Exact float64 statement of forward_interpolate (core/utils/utils.py:30-58) for the tests: numpy only, brute force.

Every source pixel (x0, y0) moves to (x1, y1) = (x0 + u, y0 + v) in float64 (numpy's int grid + float32 flow); it is a valid
point iff 0 < x1 < w and 0 < y1 < h.  wrap=True (ERP): x1 is taken modulo w (numpy's float remainder), only the y test applies,
and x distances wrap, min(|dx|, w - |dx|).  A target pixel takes the (u, v) of the valid point with the smallest squared
distance; among equally near points the lowest source raster index (np.argmin's first occurrence) -- the kernel's tie rule."""
from __future__ import annotations

import numpy as np


def moved_points(flow: np.ndarray, wrap: bool):
    """flow [2,h,w] float32 -> (x1, y1, valid) float64 / bool arrays [h*w] over the source pixels."""
    _, h, w = flow.shape
    x0, y0 = np.meshgrid(np.arange(w), np.arange(h))
    x1 = (x0 + flow[0].astype(np.float64)).reshape(-1)
    y1 = (y0 + flow[1].astype(np.float64)).reshape(-1)
    with np.errstate(invalid="ignore"):
        valid = (y1 > 0) & (y1 < h)
        if wrap:
            valid &= np.isfinite(x1)
            x1 = np.where(valid, np.mod(np.where(valid, x1, 0.0), float(w)), x1)
        else:
            valid &= (x1 > 0) & (x1 < w)
    return x1, y1, valid


def nearest(flow: np.ndarray, wrap: bool, targets=None, chunk: int = 256):
    """For target pixels (raster indices; all by default): (values [2,T] of the chosen point, its source index [T] (-1: no
    valid point), d2_min [T] its squared distance, d2_second [T] the smallest squared distance of every other point)."""
    _, h, w = flow.shape
    x1, y1, valid = moved_points(flow, wrap)
    src = np.nonzero(valid)[0]
    if targets is None:
        targets = np.arange(h * w)
    targets = np.asarray(targets)
    T = len(targets)
    vals = np.zeros((2, T), np.float32)
    idx = np.full(T, -1, np.int64)
    d_min = np.full(T, np.inf)
    d_second = np.full(T, np.inf)
    if len(src) == 0:
        return vals, idx, d_min, d_second
    px, py = x1[src], y1[src]
    fu, fv = flow[0].reshape(-1)[src], flow[1].reshape(-1)[src]
    tx, ty = (targets % w).astype(np.float64), (targets // w).astype(np.float64)
    for a in range(0, T, chunk):
        b = min(T, a + chunk)
        dx = np.abs(px[None, :] - tx[a:b, None])
        if wrap:
            dx = np.minimum(dx, w - dx)
        dy = py[None, :] - ty[a:b, None]
        d2 = dx * dx + dy * dy
        k = np.argmin(d2, axis=1)
        r = np.arange(b - a)
        idx[a:b] = src[k]
        d_min[a:b] = d2[r, k]
        vals[0, a:b], vals[1, a:b] = fu[k], fv[k]
        if d2.shape[1] > 1:
            d2[r, k] = np.inf
            d_second[a:b] = d2.min(axis=1)
    return vals, idx, d_min, d_second


def check(out: np.ndarray, flow: np.ndarray, wrap: bool, targets=None, tol: float = 1e-3):
    """Asserts the issue's bar for one image: out [2,h,w] equals the brute force exactly where the nearest point is unique by
    more than `tol` px, and everywhere the chosen value belongs to a valid point within `tol` px of the minimum distance.
    Returns the number of targets with a unique nearest point."""
    _, h, w = flow.shape
    if targets is None:
        targets = np.arange(h * w)
    vals, idx, d_min, d_second = nearest(flow, wrap, targets)
    got = out.reshape(2, -1)[:, targets]
    if np.all(idx < 0):
        assert np.all(got == 0), "no valid point: zeros"
        return 0
    unique = np.sqrt(d_second) - np.sqrt(d_min) > tol
    assert np.array_equal(got[:, unique], vals[:, unique]), int((got[:, unique] != vals[:, unique]).any(0).sum())
    x1, y1, valid = moved_points(flow, wrap)
    src = np.nonzero(valid)[0]
    fu, fv = flow[0].reshape(-1)[src], flow[1].reshape(-1)[src]
    for t in np.nonzero(~unique)[0]:
        tx, ty = targets[t] % w, targets[t] // w
        dx = np.abs(x1[src] - tx)
        if wrap:
            dx = np.minimum(dx, w - dx)
        d = np.sqrt(dx * dx + (y1[src] - ty) ** 2)
        near = d <= np.sqrt(d_min[t]) + tol
        assert np.any(near & (fu == got[0, t]) & (fv == got[1, t])), (t, got[:, t])
    return int(unique.sum())
