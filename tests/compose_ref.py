"""Float64 restatement of the chained-flow statement (include/priorflow_hip.h: pf_flow_compose, pf_track_points; DESIGN.md
section 17), the inputs its tests run on and the bounds a result is held to.  Written from the statement, not from the kernel.

One point p = (px, py), px unwrapped; a flow g [2,H,W]; optionally a mask occ [H,W] (non-zero = 1):
  g^(p): x wrapped with Python's modulo, y clamped, bilinear weights from the unclamped fraction, the u of the three non-anchor
         taps first brought to within W/2 of the anchor tap, v blended plainly;  m(p) = sum w_i occ_i over the same taps;
  p' = p + g^(p) (u NOT clipped);  new bits: 1 <=> m >= 0.5;  2 <=> py < -0.5 or py > H - 0.5;  4 <=> p or g^ not finite (the
  displacement added is then 0);  state' = state | new bits.
Dense form: p = (x, y) + f(x, y), out = f + g^(p).  Sparse form: p = pos, pos' = pos + g^(pos).

Bounds (each from the number format, none from a kernel's output):
  value   tol(p) = 4 * 2^-23 * (W + D + |g^_u| + |g^_v|) * (1 + S),  D = |p_u - x| + |p_v - y| (dense) or |px| + |py| (sparse),
          S = spread of the four un-wrapped u taps + spread of the four v taps: p is an fp32 number of that size, off by up to
          2^-23 of it, and the bilinear blend turns a position error d into a value error d * S.  u is compared PLAINLY: a
          result that lost its winding fails.
  bits    bit 0 is DECIDED when |m - 0.5| > 2 tol + 1e-6, bit 1 when py is farther than tol from -0.5 and from H - 0.5; every
          decided bit must carry the float64 decision, bit 2 always; input bits must survive; at most 1 % of a case's points
          may be undecided.  `exact=True` (inputs whose arithmetic is exact in fp32: dyadic positions and weights) decides
          every point.
`fault=` seeds one deviation from the statement into the restatement (the tests show that `check` catches each).
"""
import numpy as np

import fb_check_ref as fr

KINDS = fr.KINDS
WINDS = (0.0, 1.5, -3.0)
SHAPES = ((2, 17, 37), (2, 24, 48), (1, 64, 128))          # (B, H, W): scalar path / vec4 path / more than one block
MAX_UNDECIDED = 0.01
OCCLUDED, POLE, NONFINITE = 1, 2, 4
FAULTS = ("no_unwrap", "wrap_y", "clip_u", "not_sticky", "gt", "pole_0_Hm1", "ignore_occ")


def inputs(kind: str, B: int, H: int, W: int, wind: float):
    """(f, g [B,2,H,W] float32, state_f, occ_g [B,H,W] uint8): f = the forward flow of fb_check_ref.batch with wind * W added
    to u, g = its backward flow; occ_g = 1 on the block [H/3:H/2, W/4:W/2] and on 5 % of the pixels (default_rng(11 + b));
    state_f carries earlier bits (8 included, which no step sets) on 10 % of the pixels (default_rng(23 + b))."""
    fw, bw = fr.batch(kind, H, W)
    f = fw[:B].astype(np.float64)
    f[:, 0] += wind * W
    occ = np.zeros((B, H, W), np.uint8)
    state = np.zeros((B, H, W), np.uint8)
    for b in range(B):
        occ[b, H // 3:H // 2, W // 4:W // 2] = 1
        occ[b][np.random.default_rng(11 + b).random((H, W)) < 0.05] = 1
        g = np.random.default_rng(23 + b)
        state[b] = np.where(g.random((H, W)) < 0.10, g.integers(1, 16, (H, W)), 0).astype(np.uint8)
    return f.astype(np.float32), np.ascontiguousarray(bw[:B]), state, occ


def across_half_width(B: int, H: int, W: int):
    """(f, g [B,2,H,W] float32) of a case of this module's own: g's u swings around W/2 and is stored clipped to +-W/2, so
    neighbouring taps sit W apart and only the seam un-wrapping of the taps blends them rightly; f is a small fractional flow."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    f, g = np.zeros((B, 2, H, W)), np.zeros((B, 2, H, W))
    for b in range(B):
        u = W / 2 + 1.5 * np.sin(0.9 * x + 0.4 * y + b)
        g[b, 0] = np.mod(u + W / 2, W) - W / 2
        g[b, 1] = 0.5 * np.cos(0.3 * x)
        f[b, 0] = 0.37 + 0.01 * y
        f[b, 1] = 0.21
    return f.astype(np.float32), g.astype(np.float32)


def sample(g32, occ, px, py, fault=None):
    """g^ and m at float64 points (px, py) of one image: dict(gu, gv, m, S)."""
    g = g32.astype(np.float64)
    _, H, W = g.shape
    with np.errstate(invalid="ignore", over="ignore"):
        gx = np.mod(px, W)
        qy = np.mod(py, H) if fault == "wrap_y" else py
        fx, fy = np.floor(gx), np.floor(qy)
        xw, yw = gx - fx, qy - fy
        ok = np.isfinite(fx) & np.isfinite(fy)
        x0 = np.where(ok, fx, 0).astype(np.int64) % W
        x1 = (x0 + 1) % W
        fyc = np.clip(np.where(ok, fy, 0), -1.0e6, 1.0e6)
        if fault == "wrap_y":
            y0, y1 = fyc.astype(np.int64) % H, (fyc.astype(np.int64) + 1) % H
        else:
            y0 = np.clip(fyc, 0, H - 1).astype(np.int64)
            y1 = np.clip(fyc + 1, 0, H - 1).astype(np.int64)
        taps = ((y0, x0), (y1, x0), (y0, x1), (y1, x1))           # a (anchor), b, c, d
        wts = ((1 - xw) * (1 - yw), (1 - xw) * yw, xw * (1 - yw), xw * yw)
        us = [g[0][t] for t in taps]
        if fault != "no_unwrap":
            us = [us[0]] + [us[0] + np.mod(u - us[0] + W / 2, W) - W / 2 for u in us[1:]]
        vs = [g[1][t] for t in taps]
        gu = sum(w * u for w, u in zip(wts, us))
        gv = sum(w * v for w, v in zip(wts, vs))
        if occ is None or fault == "ignore_occ":
            m = np.zeros_like(gu)
        else:
            m = sum(w * (occ[t] != 0) for w, t in zip(wts, taps))
        S = (np.max(us, 0) - np.min(us, 0)) + (np.max(vs, 0) - np.min(vs, 0))
    return dict(gu=gu, gv=gv, m=m, S=S)


def _step(g32, occ, px, py, D, state_in, fault):
    """One image: the step of float64 points (px, py); D = the magnitude term of the bound."""
    _, H, W = g32.shape
    s = sample(g32, occ, px, py, fault)
    with np.errstate(invalid="ignore", over="ignore"):
        bad = ~(np.isfinite(px) & np.isfinite(py) & np.isfinite(s["gu"]) & np.isfinite(s["gv"]))
        gu, gv = np.where(bad, 0.0, s["gu"]), np.where(bad, 0.0, s["gv"])
        tol = 4 * 2.0 ** -23 * (W + D + np.abs(gu) + np.abs(gv)) * (1 + s["S"])
        lo, hi = (0.0, H - 1.0) if fault == "pole_0_Hm1" else (-0.5, H - 0.5)
        occl = (s["m"] > 0.5) if fault == "gt" else (s["m"] >= 0.5)
        pole = (py < lo) | (py > hi)
    bits = (occl * OCCLUDED + pole * POLE + bad * NONFINITE).astype(np.uint8)
    state = bits if fault == "not_sticky" else (state_in | bits)
    return dict(gu=gu, gv=gv, m=s["m"], tol=tol, bad=bad, bits=bits, state=state, py=py, H=H, W=W)


def _finish(r, u, v, fault):
    with np.errstate(invalid="ignore", over="ignore"):
        if fault == "clip_u":
            u = np.mod(u + r["W"] / 2, r["W"]) - r["W"] / 2
    r["out"] = np.stack([u, v])
    r["tol"] = np.asarray(r["tol"])
    return r


def reference_dense(f32, g32, state_f=None, occ_g=None, fault=None) -> dict:
    """One image: f32, g32 [2,H,W] float32, state_f, occ_g [H,W] uint8 or None.  Float64 `out` [2,H,W], `state`, and the maps
    `check` needs."""
    f = f32.astype(np.float64)
    _, H, W = f.shape
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    sf = np.zeros((H, W), np.uint8) if state_f is None else state_f
    with np.errstate(invalid="ignore", over="ignore"):
        r = _step(g32, occ_g, x + f[0], y + f[1], np.abs(f[0]) + np.abs(f[1]), sf, fault)
        return _finish(r, f[0] + r["gu"], f[1] + r["gv"], fault)


def reference_points(pos32, g32, state=None, occ=None, fault=None) -> dict:
    """One image: pos32 [N,2] float32 (x unwrapped, y), g32 [2,H,W], state [N] uint8 or None, occ [H,W] or None."""
    p = pos32.astype(np.float64)
    st = np.zeros(len(p), np.uint8) if state is None else state
    with np.errstate(invalid="ignore", over="ignore"):
        D = np.abs(p[:, 0]) + np.abs(p[:, 1])
        r = _step(g32, occ, p[:, 0], p[:, 1], D, st, fault)
        return _finish(r, p[:, 0] + r["gu"], p[:, 1] + r["gv"], fault)


def check(out, state, ref: dict, state_in=None, what="", exact=False) -> dict:
    """out [2, ...] float (the flow of the dense form, the positions (x, y) of the sparse one) and state uint8 [...] of one image
    against a reference's answer.  Prints the figures, then asserts the bounds of the module docstring; returns the figures."""
    tol, bad, H = ref["tol"], ref["bad"], ref["H"]
    out = np.asarray(out, np.float64)
    state = np.asarray(state)
    sin = np.zeros(state.shape, np.uint8) if state_in is None else np.asarray(state_in)
    good = ~bad
    with np.errstate(invalid="ignore"):
        err = np.maximum(np.abs(out[0] - ref["out"][0]), np.abs(out[1] - ref["out"][1]))       # plainly: no modulo on u
        worst = float(np.max(err[good] / tol[good])) if good.any() else 0.0
        t = np.where(good, tol, 0.0)
        dec0 = np.abs(ref["m"] - 0.5) > 2 * t + 1e-6
        dec1 = (np.abs(ref["py"] + 0.5) > t) & (np.abs(ref["py"] - (H - 0.5)) > t)
    if exact:
        dec0, dec1 = np.ones_like(dec0), np.ones_like(dec1)
    dec0, dec1 = dec0 | bad, dec1 | bad
    want = sin | ref["bits"]
    diff = state ^ want
    wrong = int(((diff & OCCLUDED != 0) & dec0).sum() + ((diff & POLE != 0) & dec1).sum() + (diff & NONFINITE != 0).sum())
    stray = int((diff & ~np.uint8(OCCLUDED | POLE | NONFINITE) != 0).sum())       # a bit nobody may touch
    lost = int(((state & sin) != sin).sum())
    figures = dict(err_over_tol=worst, undecided=float(1 - (dec0 & dec1).mean()), wrong_decided=wrong, stray=stray, lost_sticky=lost,
                   occluded=float((ref["bits"] & OCCLUDED != 0).mean()), pole=float((ref["bits"] & POLE != 0).mean()))
    print(what, figures)
    assert worst <= 1.0, (what, figures)
    held = bad & np.isfinite(ref["out"][0]) & np.isfinite(ref["out"][1])       # a non-finite sample adds nothing
    assert np.array_equal(out[:, held], ref["out"][:, held]), what
    assert figures["undecided"] <= MAX_UNDECIDED, (what, figures)
    assert wrong == 0 and stray == 0 and lost == 0, (what, figures)
    return figures
