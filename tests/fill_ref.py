"""Push-pull hole filling restated (prior-flow_amd/csrc/pf_fill.h), twice: `fill` in numpy, in fp32 with the
statement's operation order (held to the kernels bit for bit) or in float64 (for the error bound), and `fill_loops`, plain float64
loops over cells, written apart from the array form so that the two check each other.  `FAULTS` names ten planted faults of the
array form; tests/test_fill_host.py shows that each one is caught by a named check.  No GPU, no library."""
import numpy as np

FAR = 2.0 ** 30
U32 = 2.0 ** -24                      # unit roundoff of fp32
FAULTS = ("push_clamps_columns", "push_wraps_rows", "weight_not_saturated", "multiply_not_select", "one_level_too_few",
          "odd_column_pairs_with_column_0", "taps_swapped", "valid_overwritten", "divide_by_saturated", "apex_uninitialised")


def half(n):
    return max(1, (n + 1) // 2)


def levels(H, W):
    n = 0
    while H > 1 or W > 1:
        H, W, n = half(H), half(W), n + 1
    return n


def level_dims(H, W):
    """[(H_0, W_0), ..., (1, 1)]"""
    dims = [(H, W)]
    while dims[-1] != (1, 1):
        dims.append((half(dims[-1][0]), half(dims[-1][1])))
    return dims


def w0_of(src, hole, weight):
    """Level-0 weight of one image: src [C,H,W] fp32, hole [H,W] uint8, weight [H,W] fp32 or None -> fp32 [H,W]."""
    with np.errstate(invalid="ignore"):
        ok = (hole == 0) & np.all(np.abs(src) < np.float32(FAR), axis=0)
        if weight is None:
            return ok.astype(np.float32)
        ok &= np.isfinite(weight) & (weight > 0)
        return np.where(ok, np.minimum(np.where(ok, weight, 0), np.float32(1)), np.float32(0)).astype(np.float32)


def pull(v, w, fault=None):
    """(V [C,hc,wc], S [hc,wc]) of the level (v [C,h,wd], w [h,wd]); the dtype is that of w."""
    dt = w.dtype.type
    C, h, wd = v.shape
    hc, wc = half(h), half(wd)
    s = np.zeros((hc, wc), w.dtype)
    n = np.zeros((C, hc, wc), w.dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for dy in (0, 1):
            for dx in (0, 1):
                ws = np.zeros((hc, wc), w.dtype)
                vs = np.zeros((C, hc, wc), w.dtype)
                a, b = w[dy::2, dx::2], v[:, dy::2, dx::2]
                ws[:a.shape[0], :a.shape[1]] = a
                vs[:, :a.shape[0], :a.shape[1]] = b
                if fault == "odd_column_pairs_with_column_0" and dx == 1 and wd % 2 == 1 and wd > 1:
                    ws[:a.shape[0], wc - 1] = w[dy::2, 0]
                    vs[:, :a.shape[0], wc - 1] = v[:, dy::2, 0]
                take = ws > 0
                if fault == "multiply_not_select":
                    s = s + ws
                    n = n + ws * vs
                else:
                    s = np.where(take, s + ws, s)
                    n = np.where(take, n + ws * np.where(take, vs, dt(0)), n)
        sat = np.minimum(s, dt(1))
        den = sat if fault == "divide_by_saturated" else s
        V = np.where(s > 0, n / np.where(s > 0, den, dt(1)), dt(0))
    return V.astype(w.dtype), (s if fault == "weight_not_saturated" else sat)


def taps(n_fine, n_coarse, wrap, dt, fault=None):
    x = np.arange(n_fine)
    odd = (x & 1) == 1
    a = np.where(odd, (x - 1) // 2, x // 2 - 1)
    b = np.where(odd, (x + 1) // 2, x // 2)
    t = np.where(odd, dt(0.25), dt(0.75)).astype(dt)
    if fault == "taps_swapped":
        t = np.where(odd, dt(0.75), dt(0.25)).astype(dt)
    if wrap:
        return a % n_coarse, b % n_coarse, t
    return np.clip(a, 0, n_coarse - 1), np.clip(b, 0, n_coarse - 1), t


def lerp(a, b, t):
    return a + t * (b - a)


def push(U, v, w, fault=None):
    """The filled level [C,h,wd] of (v, w) from the filled level above U [C,hc,wc]."""
    dt = w.dtype.type
    C, hc, wc = U.shape
    h, wd = w.shape
    xa, xb, tx = taps(wd, wc, fault != "push_clamps_columns", dt, fault)
    ya, yb, ty = taps(h, hc, fault == "push_wraps_rows", dt, fault)
    with np.errstate(invalid="ignore", over="ignore"):
        top = lerp(U[:, ya][:, :, xa], U[:, ya][:, :, xb], tx[None, None, :])
        bot = lerp(U[:, yb][:, :, xa], U[:, yb][:, :, xb], tx[None, None, :])
        u = lerp(top, bot, ty[None, :, None])
        vs = np.where(w > 0, v, dt(0))
        soft = np.where(w <= 0, u, lerp(u, vs, w[None]))
        if fault == "valid_overwritten":
            return np.where(w > 0, lerp(u, vs, np.minimum(w, dt(0.5))[None]), u).astype(w.dtype)
        return np.where(w >= 1, v, soft).astype(w.dtype)


def fill(src, hole, weight=None, dtype=np.float32, fault=None):
    """One image.  -> dict(out [C,H,W], empty 0/1, w0, pulled [(V_l, S_l) for l = 0..L], filled [U_l for l = 0..L])."""
    w = w0_of(src, hole, weight).astype(dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.where(w > 0, src, np.float32(0)).astype(dtype) if dtype != np.float32 else src
    pulled = [(v, w)]
    n = levels(*w.shape) - (1 if fault == "one_level_too_few" else 0)
    for _ in range(max(n, 0)):
        pulled.append(pull(pulled[-1][0], pulled[-1][1], fault))
    tv, tw = pulled[-1]
    top = np.where(tw > 0, np.where(tw > 0, tv, 0), dtype(12345.0) if fault == "apex_uninitialised" else dtype(0)).astype(dtype)
    filled = [top]
    for fv, fw in pulled[-2::-1]:
        filled.insert(0, push(filled[0], fv, fw, fault))
    empty = int(not (tw > 0).any())
    return dict(out=filled[0], empty=empty, w0=pulled[0][1], pulled=pulled, filled=filled)


# ---- the same statement as loops over cells, in float64 -------------------------------------------------------------------------
def _taps1(x):
    return ((x - 1) // 2, (x + 1) // 2, 0.25) if x & 1 else (x // 2 - 1, x // 2, 0.75)


def fill_loops(src, hole, weight=None):
    """out [C,H,W] float64 and empty, cell by cell."""
    C, H, W = src.shape
    w = w0_of(src, hole, weight).astype(np.float64)
    v = np.where(w > 0, src, 0).astype(np.float64)
    pyr = [(v, w)]
    while pyr[-1][1].shape != (1, 1):
        fv, fw = pyr[-1]
        h, wd = fw.shape
        hc, wc = half(h), half(wd)
        cv, cw = np.zeros((C, hc, wc)), np.zeros((hc, wc))
        for j in range(hc):
            for i in range(wc):
                s, n = 0.0, [0.0] * C
                for dy in (0, 1):
                    for dx in (0, 1):
                        y, x = 2 * j + dy, 2 * i + dx
                        if y < h and x < wd and fw[y, x] > 0:
                            s += fw[y, x]
                            for c in range(C):
                                n[c] += fw[y, x] * fv[c, y, x]
                if s > 0:
                    for c in range(C):
                        cv[c, j, i] = n[c] / s
                cw[j, i] = min(1.0, s)
        pyr.append((cv, cw))
    tv, tw = pyr[-1]
    U = tv.copy() if tw[0, 0] > 0 else np.zeros_like(tv)
    empty = int(not tw[0, 0] > 0)
    for fv, fw in pyr[-2::-1]:
        h, wd = fw.shape
        hc, wc = U.shape[1:]
        out = np.zeros((C, h, wd))
        for y in range(h):
            ya, yb, ty = _taps1(y)
            ya, yb = max(ya, 0), min(yb, hc - 1)
            for x in range(wd):
                if fw[y, x] >= 1:
                    out[:, y, x] = fv[:, y, x]
                    continue
                xa, xb, tx = _taps1(x)
                xa, xb = xa % wc, xb % wc
                for c in range(C):
                    top = U[c, ya, xa] + tx * (U[c, ya, xb] - U[c, ya, xa])
                    bot = U[c, yb, xa] + tx * (U[c, yb, xb] - U[c, yb, xa])
                    u = top + ty * (bot - top)
                    out[c, y, x] = u if fw[y, x] <= 0 else u + fw[y, x] * (fv[c, y, x] - u)
        U = out
    return U, empty


# ---- the error bound ------------------------------------------------------------------------------------------------------------------
def bound(L, vmax, soft):
    """Bound on |fp32 - float64| of out for an image with L pulls whose valid values lie in [-vmax, vmax].  u = 2^-24.

    Every value of the pyramid is a convex combination of valid values, so it lies in [-M, M], M = vmax.
    Weights.  w0 is exact in both precisions.  S = min(1, s), s a sum of up to four positive weights: three rounded adds, so the
      relative error R of a weight grows by 3 u per pull, R(l) = 3 l u.  Without a weight map every w0 is 0 or 1, every s a small
      integer and every S exactly 0 or 1: R = 0 at every level.
    Pull.  V = n / s: each term of n carries one product and at most three adds (4 u), each term of s three adds (3 u), the
      division one rounding: 8 u M to first order.  Weights off by a relative R move a convex combination of values in [-M, M] by
      at most 2 R * 2 M.  Errors of the fine values pass through a convex combination unamplified.  So
      E_pull(l + 1) = E_pull(l) + (8 u + 4 R(l)) M.
    Push.  lerp(a, b, t) = a + t (b - a) rounds three times: |b - a| <= 2 M, |t (b - a)| <= 2 M, |result| <= M: 5 u M; a lerp is a
      convex combination, so input errors pass as their maximum.  u is two stages of lerps: E_push(l + 1) + 10 u M.  The blend
      lerp(u, v, w) adds 5 u M and, for a weight off by R(l), |v - u| R <= 2 M R(l); the branches w >= 1 and w <= 0 are its
      continuous ends.  With E_push(l + 1) >= E_pull(l):  E_push(l) = E_push(l + 1) + (15 u + 2 R(l)) M.
    Sum over the L levels: E = sum_l (23 u + 6 R(l)) M = (23 L + 9 L (L - 1) [soft only]) u M, times 1.01 for the second-order
    terms and the float64 side's own roundings (2^-53 each)."""
    per = 23.0 * L + (9.0 * L * (L - 1) if soft else 0.0)
    return 1.01 * per * U32 * vmax
