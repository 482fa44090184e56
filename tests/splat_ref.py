"""Float64 restatement of forward softmax splatting (prior-flow_amd/csrc/pf_splat.h, include/priorflow_hip.h: pf_splat_accumulate,
pf_splat_resolve), the inputs its tests run on and the bounds a result is held to.  Written from the
statement, not from the kernel.

One image, jobs j = (src [C,H,W], flow [2,H,W], metric [Cm,H,W] | None, mask [H,W] | None, tau, beta); source pixel (x, y):
  q = (x + tau u, y + tau v);  m = |metric| (Cm = 1) or the length of its two planes (Cm = 2);  w = beta exp(-min(alpha m, zmax));
  skipped when masked, or q / m / a value not finite (|q| >= 2^30 counts as not finite);
  taps (x0, x0 + 1) mod W x (y0, y0 + 1), a row outside [0, H - 1] dropped, b_k the bilinear product, b_k = 0 adds nothing;
  N_c[p] += w b_k clamp(src_c, +-vmax),  D[p] += w b_k,  cov[p] += beta b_k;  hole = cov < cmin;  out = N / D; a hole takes the fill.

Bounds per target pixel (K contributions, A = sum w, B = sum beta, eps = 2^-23, dq = 2 eps (W + max |tau u|), each from the number
formats: the integer quantum, the fp32 roundings of one product, and a position error dq that moves a bilinear weight by dq per
axis):
  tol_D   = K 2^-(S_D+1) + 6 eps D + 4 dq A           tol_cov = K 2^-(S_D+1) + 6 eps cov + 4 dq B
  tol_N   = K 2^-(S_N+1) + vmax (8 eps D + 4 dq A)    tol_out = (tol_N + |out| tol_D) / D
A hole bit is DECIDED when |cov - cmin| > tol_cov; every decided bit must be right, a decided hole must carry the fill exactly,
every other decided pixel its value within tol_out; at most 1 % of a case's pixels may be undecided.
`fault=` seeds one deviation from the statement into the restatement (the tests show that `check` catches each).

Measured on the host emulation over the whole sweep (tests/test_splat_host.py prints them): worst |err| / tol_out 0.029 (`expand`),
at most 0.061 % of a case's pixels undecided (`expand`), no decided bit wrong.  The bounds are loose by that factor because dq is
a worst case over the map.  No seeded fault slips under them, so none was tightened: the value faults land at 397 x (`no_wrap`) to
3812 x (`metric_cm1`) the bound, the two hole faults (`cov_without_beta`, `hole_on_d`) flip 743 and 265 decided bits.
"""
import numpy as np

EPS = 2.0 ** -23
FAR = 2.0 ** 30
ZMAX, CMIN, VMAX = 12.0, 2.0 ** -10, 255.0
MAX_UNDECIDED = 0.01
FAMILIES = ("pan", "integer", "seam", "poles", "expand", "collapse", "noise")
SHAPES = ((2, 17, 37), (2, 24, 48), (1, 64, 128))          # (B, H, W): element form / quad form / more than one block
TS = (0.25, 0.5, 1.0)
ALPHAS = (0.0, 0.5)
CS = (1, 3, 4)
NJOBS = (1, 2, 4)
FAULTS = ("pole_clamped", "no_wrap", "tau_u_only", "cov_without_beta", "hole_on_d", "metric_cm1")


def scales(njobs: int, H: int, W: int, vmax: float = VMAX):
    """(S_D, S_N) of a call: S_D = 62 - ceil(log2(njobs H W)), S_N = S_D - ceil(log2(vmax))."""
    n, lg, lv = njobs * H * W, 0, 0
    while (1 << lg) < n:
        lg += 1
    while 2.0 ** lv < vmax:
        lv += 1
    return 62 - lg, 62 - lg - lv


def flow_family(kind: str, H: int, W: int, rng):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    n = lambda s: rng.normal(0, s, (H, W))                 # noqa: E731
    if kind == "pan":
        u, v = 5.3 + n(.05), -1.7 + n(.05)
    elif kind == "integer":
        u, v = np.full((H, W), 3.0), np.full((H, W), -2.0)
    elif kind == "seam":
        u, v = 1.5 * W + 0.37 + n(.05), 0.4 + n(.05)
    elif kind == "poles":
        u, v = 2.0 + n(.3), np.where(y < H / 2, -(y + 2.5), (H - y) + 1.5) + n(.3)
    elif kind == "expand":
        u, v = (x - W / 2) + n(.05), (y - H / 2) + n(.05)
    elif kind == "collapse":
        u, v = (W / 3 + 0.25) - x, (H / 2 + 0.6) - y
    elif kind == "noise":
        u, v = n(6), n(6)
    else:
        raise ValueError(kind)
    return np.stack([u, v]).astype(np.float32)


def job_scalars(t: float, njobs: int):
    """(tau, beta) of the jobs of a case at time t: job 0 moves by t with weight 1 - t (1 at t = 1), job 1 by 1 - t with weight t,
    jobs 2 and 3 by t / 2 and -t / 2 with weight 1/2."""
    rows = [(t, 1.0 - t if t < 1.0 else 1.0), (1.0 - t, t), (0.5 * t, 0.5), (-0.5 * t, 0.5)]
    return rows[:njobs]


def inputs(kind: str, B: int, H: int, W: int, C: int, njobs: int, t: float, with_metric: bool, seed: int = 0, dirty: bool = True):
    """The jobs of one case: a list of dicts src [B,C,H,W], flow [B,2,H,W] float32, metric [B,Cm,H,W] | None (Cm = 2 on the odd
    jobs), mask [B,H,W] uint8 | None (on the jobs with (j + C) even), tau, beta.  Frames uniform in [0, 255], the metric uniform
    in [0, 40], generators default_rng(seed + 101 j + 7 b).  dirty: the last job carries a NaN and an inf flow, a flow that lands
    beyond 2^30, an inf value and a value beyond vmax at fixed pixels."""
    jobs = []
    for j, (tau, beta) in enumerate(job_scalars(t, njobs)):
        cm = 2 if j % 2 else 1
        src = np.empty((B, C, H, W), np.float32)
        flow = np.empty((B, 2, H, W), np.float32)
        metric = np.empty((B, cm, H, W), np.float32) if with_metric else None
        mask = np.zeros((B, H, W), np.uint8) if (j + C) % 2 == 0 else None
        for b in range(B):
            rng = np.random.default_rng(seed + 101 * j + 7 * b)
            flow[b] = flow_family(kind, H, W, rng)
            src[b] = rng.uniform(0, 255, (C, H, W))
            m = rng.uniform(0, 40, (cm, H, W))
            if with_metric:
                metric[b] = m if cm == 1 else m * np.sign(rng.normal(size=m.shape)) / np.sqrt(2)
            k = rng.random((H, W)) < 0.05
            if mask is not None:
                mask[b][k] = 3
                mask[b, H // 3:H // 2, W // 4:W // 2] = 1
        if dirty and j == njobs - 1:
            flow[0, 0, 1, 2] = np.nan
            flow[0, 1, 2, 3] = np.inf
            flow[0, 0, 3, 4] = 3.0e9 / max(abs(tau), 0.25)
            src[0, C - 1, 4, 5] = np.inf
            src[0, 0, 5, 6] = 1.0e4
        jobs.append(dict(src=src, flow=flow, metric=metric, mask=mask, tau=float(np.float32(tau)), beta=float(np.float32(beta))))
    return jobs


# ---- cases for the code that exists only in pf_splat.hip: the LDS window of pf_splat_acc_kernel ------------------------------------
# The sweep above reaches the window's branches at (1, 64, 128) only and never an unplaced centre, a map narrower than the window,
# a second image beside a second tile column, or a third column (tests/launch_paths.py: splat_window_paths says what a case
# reaches; tests/test_launch_paths.py shows it for these and for the sweep).  Every flow value here is a multiple of 1/4, so with
# tau in {1/4, 1/2, 1} and the 1/8 of a four-job case every landing, and with it the window-or-direct choice of every tap, is exact
# in fp32.
DEVICE_SHAPES = ((3, 20, 200), (2, 12, 72), (2, 9, 80), (2, 16, 65))     # four columns / W < window / W = window / one-pixel column
DEVICE_FAMILIES = ("centre_bad", "torn_x", "torn_y", "margin", "back")
DEVICE_SETTINGS = ((0.5, 0.0, 3, 2), (1.0, 0.5, 4, 4), (0.25, 0.0, 1, 1))          # (t, alpha, C, njobs); two jobs: the blend fill
CENTRE_FAR = ("centre_far", (3, 20, 200), 0.5, 0.0, 3, 2)                 # held to the emulation's bits only (see device_paths)
TILE_Y, TILE_X = 8, 64                                                    # pf_splat.hip kTileY, kTileX


def tile_centres(H: int, W: int):
    """(cy, cx) of every tile of pf_splat_acc_kernel, row-major: min(ty0 + 4, H - 1), min(tx0 + 32, W - 1)."""
    return [(min(ty + TILE_Y // 2, H - 1), min(tx + TILE_X // 2, W - 1)) for ty in range(0, H, TILE_Y) for tx in range(0, W, TILE_X)]


def device_flow(kind: str, H: int, W: int, b: int, j: int, tau: float):
    """Flow [2,H,W] float32 of image b, job j: a family in tile-relative coordinates, plus an integer shift per image (3 b, -b) and
    a quarter-step shift per job (j / 4, j / 4)."""
    y, x = np.mgrid[0:H, 0:W]
    ry, rx = y % TILE_Y, x % TILE_X
    zero = np.zeros((H, W))
    if kind in ("centre_bad", "centre_far"):
        u, v = zero + 5.25, zero - 1.75
    elif kind == "torn_x":
        u, v = np.where(rx < TILE_X // 2, 3.25, 40.5), zero + 0.75
    elif kind == "torn_y":
        u, v = zero + 2.5, np.where(ry < TILE_Y // 2, 1.25, 9.5)
    elif kind == "margin":
        u = np.where(rx < 8, -8.5, np.where(rx >= TILE_X - 8, 8.5, 0.0))
        v = np.where(ry < 2, -4.5, np.where(ry >= TILE_Y - 2, 4.5, 0.0))
    elif kind == "back":
        u, v = zero - 2.25 * W - 0.5, zero + 0.5
    else:
        raise ValueError(kind)
    f = np.stack([u + 3 * b + 0.25 * j, v - b + 0.25 * j]).astype(np.float32)
    assert np.array_equal(f * 4, np.rint(f * 4))
    if kind == "centre_bad":        # the tile centres carry NaN, +inf, a landing beyond 2^30 and -inf in turn
        bad = ((0, np.nan), (1, np.inf), (0, 3.0e9 / max(abs(tau), 0.25)), (1, -np.inf))
        for k, (cy, cx) in enumerate(tile_centres(H, W)):
            c, value = bad[(k + b + j) % 4]
            f[c, cy, cx] = value
    elif kind == "centre_far":      # finite and inside [2^28, 2^30) at tau >= 1/2: the pixel is splatted, its tile's window is not placed
        for cy, cx in tile_centres(H, W):
            f[0, cy, cx] = 6.0e8
    return f


def device_inputs(kind: str, B: int, H: int, W: int, C: int, njobs: int, t: float, with_metric: bool):
    """The jobs of a DEVICE_PATHS case: frames, metrics and masks as `inputs` makes them, the flows of device_flow."""
    jobs = inputs("integer", B, H, W, C, njobs, t, with_metric, dirty=False)
    for j, q in enumerate(jobs):
        for b in range(B):
            q["flow"][b] = device_flow(kind, H, W, b, j, q["tau"])
    return jobs


def device_paths():
    """(kind, shape, t, alpha, C, njobs) of every case for the window.  `centre_far` is not among them: a centre that lands in
    [2^28, 2^30) is a pixel with |tau u| = 3e8, which takes dq = 2 eps (W + max |tau u|) to 72 pixels and leaves the float64
    restatement undecided on every pixel; that case (CENTRE_FAR) is held to the emulation's bits alone."""
    return [(k, s) + st for k in DEVICE_FAMILIES for s in DEVICE_SHAPES for st in DEVICE_SETTINGS]


def fill_blend(f0, f1, t):
    """(1 - t) f0 + t f1 as the kernel evaluates it: every step a rounded fp32 operation."""
    t = np.float32(t)
    return ((np.float32(1) - t) * f0.astype(np.float32) + t * f1.astype(np.float32)).astype(np.float32)


def reference(jobs, b: int, alpha: float, zmax: float = ZMAX, vmax: float = VMAX, cmin: float = CMIN, fault=None) -> dict:
    """Image b of a case in float64: out [C,H,W], hole, and the maps `check` needs."""
    C, H, W = jobs[0]["src"].shape[1:]
    HW = H * W
    SD, SN = scales(len(jobs), H, W, vmax)
    N, D, cov, K, A, Bs = np.zeros((C, HW)), np.zeros(HW), np.zeros(HW), np.zeros(HW), np.zeros(HW), np.zeros(HW)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    umax = 0.0
    alpha = float(np.float32(alpha))
    with np.errstate(invalid="ignore", over="ignore"):
        for q in jobs:
            tau, beta = q["tau"], q["beta"]
            fl = q["flow"][b].astype(np.float64)
            src = q["src"][b].astype(np.float64)
            qx = x + tau * fl[0]
            qy = y + (fl[1] if fault == "tau_u_only" else tau * fl[1])
            ok = (np.abs(qx) < FAR) & (np.abs(qy) < FAR) & np.isfinite(src).all(0)
            if q["mask"] is not None:
                ok &= q["mask"][b] == 0
            w = np.full((H, W), beta)
            if q["metric"] is not None:
                m = q["metric"][b].astype(np.float64)
                mm = np.abs(m[0]) if (m.shape[0] == 1 or fault == "metric_cm1") else np.sqrt(m[0] ** 2 + m[1] ** 2)
                ok &= np.isfinite(mm)
                if alpha > 0:
                    w = beta * np.exp(-np.minimum(alpha * np.where(np.isfinite(mm), mm, 0.0), zmax))
            umax = max(umax, float(np.max(np.abs(tau * fl[0][ok]), initial=0.0)))
            val = np.clip(np.where(np.isfinite(src), src, 0.0), -vmax, vmax)
            qx, qy = np.where(ok, qx, 0.0), np.where(ok, qy, 0.0)
            x0, y0 = np.floor(qx), np.floor(qy)
            fx, fy = qx - x0, qy - y0
            for dy in (0, 1):
                for dx in (0, 1):
                    bk = (fx if dx else 1 - fx) * (fy if dy else 1 - fy)
                    yy, xx = (y0 + dy).astype(np.int64), (x0 + dx).astype(np.int64)
                    keep = ok & (bk > 0)
                    if fault == "pole_clamped":
                        yy = np.clip(yy, 0, H - 1)
                    else:
                        keep &= (yy >= 0) & (yy < H)
                    if fault == "no_wrap":
                        keep &= (xx >= 0) & (xx < W)
                    idx = (yy * W + np.mod(xx, W))[keep]
                    wb = (w * bk)[keep]
                    D += np.bincount(idx, wb, HW)
                    cov += np.bincount(idx, (bk if fault == "cov_without_beta" else beta * bk)[keep], HW)
                    K += np.bincount(idx, None, HW)
                    A += np.bincount(idx, w[keep], HW)
                    Bs += np.bincount(idx, np.full(idx.shape, beta), HW)
                    for c in range(C):
                        N[c] += np.bincount(idx, wb * val[c][keep], HW)
    dq = 2 * EPS * (W + umax)
    tol_d = K * 2.0 ** -(SD + 1) + 6 * EPS * D + 4 * dq * A
    tol_cov = K * 2.0 ** -(SD + 1) + 6 * EPS * cov + 4 * dq * Bs
    tol_n = K * 2.0 ** -(SN + 1) + vmax * (8 * EPS * D + 4 * dq * A)
    hole = (D < cmin) if fault == "hole_on_d" else (cov < cmin)
    safe = np.where(D > 0, D, 1.0)
    out = np.where(hole, 0.0, N / safe)
    tol_out = (tol_n + np.abs(out) * tol_d) / safe
    shp = lambda a: a.reshape(a.shape[:-1] + (H, W))       # noqa: E731
    return dict(out=shp(out), hole=shp(hole), cov=shp(cov), D=shp(D), N=shp(N), K=shp(K), tol_out=shp(tol_out), tol_cov=shp(tol_cov),
                decided=shp(np.abs(cov - cmin) > tol_cov), cmin=cmin, SD=SD, SN=SN)


def check(out, hole, ref: dict, fill=None, what="") -> dict:
    """out [C,H,W] float32 and hole [H,W] uint8 of one image against the reference's answer; fill [C,H,W] float32 (what a hole
    takes) or None (0).  Prints the figures, then asserts the bounds of the module docstring; returns the figures."""
    out64 = np.asarray(out, np.float64)
    hole = np.asarray(hole) != 0
    dec = ref["decided"]
    wrong = int(((hole != ref["hole"]) & dec).sum())
    val = dec & ~ref["hole"] & ~hole
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio =np.abs(out64 - ref["out"]) / ref["tol_out"]
    worst = float(np.max(ratio[:, val])) if val.any() else 0.0
    filled = np.zeros_like(np.asarray(out, np.float32)) if fill is None else fill
    h = hole & ref["hole"]
    fill_ok = bool(np.array_equal(np.asarray(out, np.float32)[:, h].view(np.uint32), filled[:, h].view(np.uint32)))
    figures = dict(err_over_tol=worst, undecided=float(1 - dec.mean()), wrong_decided=wrong, holes=float(ref["hole"].mean()),
                   fill_ok=fill_ok, finite=bool(np.isfinite(out64[:, ~hole]).all()))
    print(what, figures)
    assert figures["finite"], (what, figures)
    assert worst <= 1.0, (what, figures)
    assert figures["undecided"] <= MAX_UNDECIDED, (what, figures)
    assert wrong == 0, (what, figures)
    assert fill_ok, (what, figures)
    return figures


def sweep():
    """(kind, shape, t, alpha, C, njobs) of every case; `expand` at t = 1.0 is left out (its 2x lattice puts more than 1 % of
    the coverages right at cmin)."""
    return [(k, s, t, a, C, nj) for k in FAMILIES for s in SHAPES for t in TS for a in ALPHAS for C in CS for nj in NJOBS
            if not (k == "expand" and t == 1.0)]
