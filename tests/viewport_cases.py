"""Inputs, runners and the derived per-pixel bounds of the viewport / cube map tests.  Not collected;
shared by tests/test_viewport_host.py (host emulation) and tests/test_hip_viewport.py (device).

The bounds.  U = 2^-24 is fp32's unit roundoff; the statement (tests/viewport_ref.py) is evaluated in float64 on the fp32 inputs,
so only the kernel's own arithmetic is budgeted.  Every constant below counts roundings of csrc/pf_viewport.h's expressions or is
a library function's documented error; none is taken from an observed error.

  ray        a = (j - c_x) / f, b = -(i - c_y) / f: one rounding each (the differences are exact).  A component of d = R (1, a, b)
             is three products of entries |R| <= 1 and two sums: |dd| <= 4 U L1, L1 = 1 + |a| + |b|.
  theta      atan2f(d_y, d_x): moving (d_x, d_y) by dd each turns the angle by at most sqrt(2) dd / rho, rho = hypot(d_x, d_y);
             atan2f itself is budgeted at 4 ulp = 8 U |theta| (HIP documents 2 ulp, glibc below 1).
  phi        atan2f(d_z, rho~): rho~ carries sqrt(2) dd from its inputs and 2 U rho from two squares, a sum and a root; the
             angle of (rho~, d_z) moves by at most (dd rho + (sqrt(2) dd + 2 U rho) |d_z|) / |d|^2, plus 8 U |phi|.
             (asin(d_z / |d|) is the same angle; this form keeps the budget finite at the poles.)
  position   m = (theta / 2 pi + 1/2) W - 1/2 is a quotient <= 1/2, a sum <= 1, a product and a difference <= W, and the wrap
             of a negative m adds W once more: dm = W dtheta / (2 pi) + 5 U W; dn = H dphi / pi + 4 U H.
  image      bilinear interpolation is continuous and piecewise linear, so to first order the value moves by dm gx + dn gy with
             gx (gy) the largest horizontal (vertical) tap difference in the 2x2 cell and the cells beside it (a position error
             may cross into the neighbour); the mix is two weight factors, their product, the product with the tap and three
             sums: 8 U max|tap|.
  flow       p^ = d / |d|: 2 dd / |d| + 3 U.  A sphere point s(m', n'): theta' is a sum, a sum, a quotient, a difference and a
             product, dtheta' = 4 pi U (|m'| + 1) / W + 3 U |theta'|, dphi' = 2 pi U (|n'| + 1) / H + 3 U |phi'|; sinf / cosf at
             4 ulp of a value <= 1 (8 U each) and one product: de = dtheta' + dphi' + 17 U per component; D = e - s carries both
             and U |D|.  q = p^ + sum w_k D_k: dq = dp^ + max_k dD_k + dm Gx + dn Gy + 8 U max_k |D_k| + U |q|, with Gx, Gy the
             tap differences of D as for an image.  c = R^T q: dc = 3 dq + 3 sqrt(3) U |q|.  x = c_x + f c_r / c_f moves by
             f dc (|c_f| + |c_r|) / c_f^2 -- the factor f |q| / q_f^2 that min_forward bounds -- plus 3 U |x - c_x| + U max(|x|, c_x).
             out = proj(q) - proj(p^): both budgets and U |out|.
  cube       d = s(m, n) as above (ds); proj with entries 0, +-1 is a selection: dx = f ds (|c_f| + |c_r|) / c_f^2 + 3 U |x - c| +
             U max(|x|, c), then the image rule on the face.
"""
import ctypes

import numpy as np
import torch

import viewport_ref as vr

U = 2.0 ** -24
MIN_FORWARD = float(np.cos(np.radians(85.0)))
PANORAMAS = ((32, 64), (40, 72))
VIEW_SIZES = ((17, 23), (16, 16))
NEAR = np.pi / 2 - 0.1
# (yaw, pitch, roll, fov_x_deg)
VIEW_SETS = {
    1: ((0.0, 0.0, 0.0, 100.0),),
    4: ((np.pi, 0.0, 0.0, 100.0), (0.0, NEAR, 0.0, 100.0), (0.0, -NEAR, 0.0, 120.0), (0.7, -0.4, 0.3, 30.0)),
    7: ((0.0, 0.0, 0.0, 100.0), (np.pi, 0.0, 0.0, 120.0), (0.3, NEAR, 0.0, 30.0), (-1.0, -NEAR, 0.0, 100.0), (0.7, -0.4, 0.3, 100.0),
        (-2.1, 0.5, -1.0, 120.0), (2.5, 1.0, 0.6, 30.0)),
}
# the four views of the second-order check: clear of the pole caps, and no 120 degree view -- at 32 rows the edge pixels of such a
# view are not yet in the asymptotic regime (the float64 statement's ratios there: 0.34 for the first halving, 0.24 for the second)
OFF_POLE_VIEWS = ((0.0, 0.0, 0.0, 100.0), (np.pi, 0.0, 0.0, 100.0), (2.5, 0.6, 0.6, 100.0), (2.5, 1.0, 0.6, 30.0))
IMAGE_FORMS = ((1, 1, "f32"), (2, 3, "f32"), (2, 3, "u8"), (1, 1, "u8"))       # (B, C, form)
FLOW_KINDS = ("zero", "u3", "u_half", "smooth", "smooth_nan")
CUBE_SIZES = (8, 12)
# directions with an exact tie of the largest |component| (a pixel centre never has one: cos(pi/4) != sin(pi/4) in either precision)
TIES = ((1.0, 1.0, 0.0), (1.0, -1.0, 0.0), (-1.0, 1.0, 0.5), (1.0, 0.0, 1.0), (0.0, 1.0, -1.0), (-1.0, -1.0, 1.0), (1.0, 1.0, 1.0),
        (-1.0, -1.0, -1.0), (0.0, -1.0, 1.0), (-0.5, 0.25, -0.5), (0.0, 0.0, 0.0))


def rows_of(V, h, w, fault=None):
    """The float64 rows of view set V at h x w, and the fp32 table the C-ABI takes."""
    rows = np.array([vr.viewport_row(y, p, r, fov, h, w, fault) for y, p, r, fov in VIEW_SETS[V]])
    return rows, vr.table32(rows)


def make_image(B, C, H, W, seed):
    """Smooth structure plus some noise, 0..255, fp32 (periodic in m as a panorama is)."""
    rng = np.random.default_rng(seed)
    n, m = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    out = np.empty((B, C, H, W), np.float32)
    for b in range(B):
        for c in range(C):
            a, k, p = rng.uniform(0, 2 * np.pi), rng.integers(1, 4), rng.uniform(0, 2 * np.pi)
            out[b, c] = 127.5 + 90 * np.sin(2 * np.pi * k * m / W + a) * np.cos(np.pi * n / H + p) + rng.uniform(-25, 25, (H, W))
    return np.clip(out, 0, 255)


def make_u8(B, C, H, W, seed):
    return np.ascontiguousarray(np.round(make_image(B, C, H, W, seed)).astype(np.uint8).transpose(0, 2, 3, 1))


def make_flow(kind, B, H, W, seed=0):
    """ERP flows [B,2,H,W] fp32.  "smooth": |u| up to 25, |v| up to 8; v does not vanish at the pole rows, so end points cross both
    poles, and with u up to 140 degrees of longitude at W = 64 a share of the end points lands behind a view's camera."""
    flow = np.zeros((B, 2, H, W), np.float32)
    n, m = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    if kind == "u3":
        flow[:, 0] = 3.0
    elif kind == "u_half":
        flow[:, 0] = W / 2 - 0.25
    elif kind in ("smooth", "smooth_nan"):
        for b in range(B):
            a = 0.9 * (seed + b) + 0.4
            flow[b, 0] = 25 * np.sin(2 * np.pi * m / W + a) * np.cos(np.pi * n / H + 0.5 * a)
            flow[b, 1] = 8 * np.cos(4 * np.pi * m / W + 1.3 * a)
        if kind == "smooth_nan":
            flow[:, 0, H // 2 - 3:H // 2 + 2, W // 2 - 4:W // 2 + 3] = np.nan
            flow[0, 1, 2:5, 1:4] = np.inf
            flow[-1, 0, H - 4:H - 1, W - 3:] = -np.inf
    elif kind != "zero":
        raise ValueError(kind)
    return flow


def make_faces(B, C, s, seed):
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(s), np.arange(s), indexing="ij")
    out = np.empty((B, 6, C, s, s), np.float32)
    for idx in np.ndindex(B, 6, C):
        a, p = rng.uniform(0.5, 2.0), rng.uniform(0, 2 * np.pi)
        out[idx] = 100 + 80 * np.sin(a * x / s * np.pi + p) * np.cos(a * y / s * np.pi) + rng.uniform(-10, 10, (s, s))
    return out


# ---- runners: outputs between guard rows that must stay untouched ------------------------------------------------------------
GUARD = 64          # elements before and after every output


def _guarded(shape, dtype, device):
    n = int(np.prod(shape))
    fill = 0xA5 if dtype == torch.uint8 else -12345.0
    big = torch.full((GUARD + n + GUARD,), fill, dtype=dtype, device=device)
    return big, big[GUARD:GUARD + n].view(*shape), fill


def _unguard(big, fill):
    b = big.cpu()
    assert bool((b[:GUARD] == fill).all()) and bool((b[-GUARD:] == fill).all()), "memory beside an output was written"
    return b[GUARD:-GUARD]


def _table(lib, t32):
    return lib.view_table(np.asarray(t32, np.float32).reshape(-1, 12).tolist())


def run_image(lib, x, t32, device="cpu"):
    """x: fp32 [B,C,H,W] or uint8 [B,H,W,C] numpy -> the views as numpy."""
    V, h, w = len(t32), int(t32[0][10]), int(t32[0][11])
    xt = torch.from_numpy(np.ascontiguousarray(x)).to(device)
    if x.dtype == np.uint8:
        B, H, W, C = x.shape
        shape = (B, V, h, w, C)
    else:
        B, C, H, W = x.shape
        shape = (B, V, C, h, w)
    big, out, fill = _guarded(shape, xt.dtype, device)
    lib.viewport_image(xt, _table(lib, t32), out)
    return _unguard(big, fill).view(*shape).numpy()


def run_flow(lib, flow, t32, min_forward=MIN_FORWARD, device="cpu"):
    V, h, w = len(t32), int(t32[0][10]), int(t32[0][11])
    B = flow.shape[0]
    ft = torch.from_numpy(np.ascontiguousarray(flow)).to(device)
    bo, out, fo = _guarded((B, V, 2, h, w), torch.float32, device)
    bv, valid, fv = _guarded((B, V, h, w), torch.uint8, device)
    lib.viewport_flow(ft, _table(lib, t32), out, valid, min_forward)
    return _unguard(bo, fo).view(B, V, 2, h, w).numpy(), _unguard(bv, fv).view(B, V, h, w).numpy()


def run_cube(lib, faces, H, W, device="cpu"):
    B, _, C, s, _ = faces.shape
    ft = torch.from_numpy(np.ascontiguousarray(faces)).to(device)
    big, out, fill = _guarded((B, C, H, W), torch.float32, device)
    lib.cubemap_to_erp(ft, out)
    return _unguard(big, fill).view(B, C, H, W).numpy()


def emu_faces(emu, dirs):
    f = emu._dll.pf_emu_cube_face
    f.argtypes, f.restype = [ctypes.c_float] * 3, ctypes.c_int
    return np.array([f(*d) for d in dirs])


# ---- bounds --------------------------------------------------------------------------------------------------------------------
def position_budget(row, H, W):
    """(dm, dn, dd, |d|) [h,w] of one view: the fp32 budget of the ray's ERP position."""
    d = vr.rays(row)
    R = np.asarray(row, np.float64)[:9].reshape(3, 3)
    cam = d @ R                                               # (1, a, b) again
    L1 = 1 + np.abs(cam[..., 1]) + np.abs(cam[..., 2])
    dd = 4 * U * L1
    rho = np.hypot(d[..., 0], d[..., 1])
    nd = np.linalg.norm(d, axis=-1)
    theta, phi = np.arctan2(d[..., 1], d[..., 0]), np.arctan2(d[..., 2], rho)
    dtheta = np.sqrt(2) * dd / rho + 8 * U * np.abs(theta)
    dphi = (dd * rho + (np.sqrt(2) * dd + 2 * U * rho) * np.abs(d[..., 2])) / nd ** 2 + 8 * U * np.abs(phi)
    return W * dtheta / (2 * np.pi) + 5 * U * W, H * dphi / np.pi + 4 * U * H, dd, nd


def cell_gradients(F, x0, y0, wrap):
    """F [..., Hh, Ww, K]; x0, y0 integer arrays (floor of the position, y unclamped) -> (gx, gy): the largest |difference| of
    horizontally (vertically) adjacent taps over the channels, in the 2x2 cell and the cells beside it.  NaN entries are skipped."""
    Hh, Ww = F.shape[-3], F.shape[-2]
    with np.errstate(invalid="ignore"):
        nxt = np.roll(F, -1, axis=-2) if wrap else np.concatenate([F[..., 1:, :], F[..., -1:, :]], axis=-2)
        DX = np.fmax.reduce(np.abs(nxt - F), axis=-1)                      # difference starting at column x
        DY = np.fmax.reduce(np.abs(np.concatenate([F[..., 1:, :, :], F[..., -1:, :, :]], axis=-3) - F), axis=-1)
    DX, DY = np.nan_to_num(DX), np.nan_to_num(DY)
    cx = (lambda a: a % Ww) if wrap else (lambda a: np.clip(a, 0, Ww - 1))
    cy = lambda a: np.clip(a, 0, Hh - 1)                      # noqa: E731
    gx = gy = 0.0
    for dy in (0, 1):
        for dx in (-1, 0, 1):
            gx = np.maximum(gx, DX[..., cy(y0 + dy), cx(x0 + dx)])
    for dy in (-1, 0, 1):
        for dx in (0, 1):
            gy = np.maximum(gy, DY[..., cy(y0 + dy), cx(x0 + dx)])
    return gx, gy


def _cell(m, n, W):
    return np.floor(np.mod(m, W)).astype(np.int64), np.floor(n).astype(np.int64)


def image_bound(x, rows):
    """Per-pixel bound [B,V,C,h,w] of pf_viewport_image on x [B,C,H,W] (float64 values of the fp32 or byte input)."""
    x = np.asarray(x, np.float64)
    B, C, H, W = x.shape
    out = []
    for r in rows:
        dm, dn, _, _ = position_budget(r, H, W)
        m, n = vr.erp_of(vr.rays(r), H, W)
        x0, y0 = _cell(m, n, W)
        gx, gy = cell_gradients(x[..., None], x0, y0, wrap=True)          # [B,C,h,w]
        ys, xs, _, _ = vr.wraptaps(m, n, H, W)
        out.append(dm * gx + dn * gy + 8 * U * np.abs(x[:, :, ys, xs]).max(2))
    return np.stack(out, 1)


def _proj_budget(c, dc, f, cx, cy):
    """Budget of proj's x and y for camera coordinates c [...,3] known to dc."""
    cf = np.abs(c[..., 0])
    with np.errstate(divide="ignore", invalid="ignore"):
        tx, ty = f * c[..., 1] / c[..., 0], f * c[..., 2] / c[..., 0]
        bx = f * dc * (cf + np.abs(c[..., 1])) / cf ** 2 + 3 * U * np.abs(tx) + U * np.maximum(np.abs(cx + tx), cx)
        by = f * dc * (cf + np.abs(c[..., 2])) / cf ** 2 + 3 * U * np.abs(ty) + U * np.maximum(np.abs(cy - ty), cy)
    return bx, by


def flow_bound(flow, rows):
    """Per-pixel bound [B,V,2,h,w] of pf_viewport_flow (meaningful where the statement's valid is 1)."""
    flow = np.asarray(flow, np.float64)
    B, _, H, W = flow.shape
    finite = np.isfinite(flow).all(1)
    safe = np.where(finite[:, None], flow, 0.0)
    n, m = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")

    def dsphere(mm, nn):
        theta = ((mm + 0.5) / W - 0.5) * 2 * np.pi
        phi = (0.5 - (nn + 0.5) / H) * np.pi
        return (4 * np.pi * U * (np.abs(mm) + 1) / W + 3 * U * np.abs(theta)) + (2 * np.pi * U * (np.abs(nn) + 1) / H + 3 * U * np.abs(phi)) + 17 * U

    D = vr.displacement(safe)                                              # [B,H,W,3]
    dD = dsphere(m + safe[:, 0], np.clip(n + safe[:, 1], -0.5, H - 0.5)) + dsphere(m, n)[None] + U * np.abs(D).max(-1)
    Dn = np.where(finite[..., None], D, np.nan)
    out = []
    for r in rows:
        R, f, h, w, cx, cy = vr._view(r)
        dm, dn, dd, nd = position_budget(r, H, W)
        d = vr.rays(r)
        p = d / nd[..., None]
        mm, nn = vr.erp_of(d, H, W)
        x0, y0 = _cell(mm, nn, W)
        Gx, Gy = cell_gradients(Dn, x0, y0, wrap=True)                     # [B,h,w]
        ys, xs, ws, _ = vr.wraptaps(mm, nn, H, W)
        q = p[None] + (D[:, ys, xs] * ws[None, ..., None]).sum(1)
        dp = 2 * dd / nd + 3 * U
        dq = dp[None] + dD[:, ys, xs].max(1) + dm * Gx + dn * Gy + 8 * U * np.abs(D[:, ys, xs]).max((1, 4)) \
            + U * np.linalg.norm(q, axis=-1)
        bqx, bqy = _proj_budget(q @ R, 3 * dq + 3 * np.sqrt(3) * U * np.linalg.norm(q, axis=-1), f, cx, cy)
        bpx, bpy = _proj_budget(p @ R, 3 * dp + 3 * np.sqrt(3) * U, f, cx, cy)
        qx, qy, _ = vr.proj(q, r)
        px, py, _ = vr.proj(p, r)
        out.append(np.stack([bqx + bpx[None] + U * np.abs(qx - px[None]), bqy + bpy[None] + U * np.abs(qy - py[None])], 1))
    return np.stack(out, 1)


def cube_bound(faces, H, W):
    """Per-pixel bound [B,C,H,W] of pf_cubemap_to_erp."""
    faces = np.asarray(faces, np.float64)
    B, _, C, s, _ = faces.shape
    n, m = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    theta, phi = ((m + 0.5) / W - 0.5) * 2 * np.pi, (0.5 - (n + 0.5) / H) * np.pi
    ds = (4 * np.pi * U * (m + 1) / W + 3 * U * np.abs(theta)) + (2 * np.pi * U * (n + 1) / H + 3 * U * np.abs(phi)) + 17 * U
    face, px, py = vr.cube_positions(s, H, W)
    d = vr.sphere(m, n, H, W)
    rows = vr.cube_rows(s)
    c = np.zeros((H, W, 3))
    for k in range(6):
        c = np.where((face == k)[..., None], d @ rows[k][:9].reshape(3, 3), c)
    c0 = (s - 1) / 2.0
    bx, by = _proj_budget(c, ds, s / 2.0, c0, c0)
    x0, y0 = np.floor(px).astype(np.int64), np.floor(py).astype(np.int64)
    F = faces[:, face].transpose(0, 3, 1, 2, 4, 5)                          # [B,C,H,W,s,s]
    gx = gy = tap = 0.0
    cl = lambda a: np.clip(a, 0, s - 1)                       # noqa: E731
    hh, ww = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    at = lambda yy, xx: F[:, :, hh, ww, cl(yy), cl(xx)]       # noqa: E731  [B,C,H,W]
    for dy in (-1, 0, 1, 2):
        for dx in (-1, 0, 1, 2):
            if dx < 2 and 0 <= dy <= 1:
                gx = np.maximum(gx, np.abs(at(y0 + dy, x0 + dx + 1) - at(y0 + dy, x0 + dx)))
            if dy < 2 and 0 <= dx <= 1:
                gy = np.maximum(gy, np.abs(at(y0 + dy + 1, x0 + dx) - at(y0 + dy, x0 + dx)))
            if 0 <= dy <= 1 and 0 <= dx <= 1:
                tap = np.maximum(tap, np.abs(at(y0 + dy, x0 + dx)))
    return bx * gx + by * gy + 8 * U * tap


# ---- comparisons ---------------------------------------------------------------------------------------------------------------
def check_values(got, want, bound, what, mask=None):
    """Assert |got - want| <= bound where mask (default: everywhere); prints and returns the worst ratio."""
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.abs(np.asarray(got, np.float64) - want) / bound
    ratio = np.where(np.abs(np.asarray(got, np.float64) - want) == 0, 0.0, ratio)
    if mask is not None:
        ratio = np.where(mask, ratio, 0.0)
    worst = float(np.nan_to_num(ratio, nan=np.inf).max()) if ratio.size else 0.0
    print(f"[viewport] {what}: worst |err| / bound {worst:.3f}")
    assert worst <= 1.0, (what, worst)
    return worst


def check_bytes(got, val, bound, what):
    """Bytes against the float64 value `val` before rounding: equal to floor(val + 1/2), or off by one where val lies within
    `bound` of a half-integer.  Prints the share of such pixels."""
    want = np.clip(np.floor(val + 0.5), 0, 255)
    diff = np.abs(got.astype(np.int64) - want.astype(np.int64))
    near = np.abs(val - np.floor(val) - 0.5) <= bound
    share = float(near.mean())
    print(f"[viewport] {what}: bytes that differ {int((diff > 0).sum())} of {diff.size}; share within the bound of a half-integer {share:.2e}")
    assert diff.max() <= 1 and not (diff > 0)[~near].any(), (what, int(diff.max()), int(((diff > 0) & ~near).sum()))
    return share


def check_flow(got, got_valid, flow, rows, what, min_forward=MIN_FORWARD, ref=None):
    """pf_viewport_flow's outputs against the statement: valid equal except where the float64 cosine lies within 1e-5 of
    min_forward (at most 0.5 % of the case, the statement alone must stay below that), values under the bound where both are
    valid, exactly (0, 0) where the output is not valid.  `ref` overrides the statement's result (seeded faults)."""
    want, wvalid, cosine = vr.view_flow(flow, rows, min_forward) if ref is None else ref
    bound = flow_bound(flow, rows)
    with np.errstate(invalid="ignore"):
        near = np.abs(cosine - min_forward) <= 1e-5
    share = float(np.nan_to_num(near).mean())
    print(f"[viewport] {what}: valid {int(wvalid.sum())} of {wvalid.size}; within 1e-5 of min_forward {share:.2e}")
    assert share <= 0.005, (what, share)
    assert np.array_equal(got_valid[~near], wvalid[~near]), (what, "valid differs", int((got_valid != wvalid)[~near].sum()))
    assert set(np.unique(got_valid)) <= {0, 1}
    off = got_valid == 0
    assert not got[:, :, 0][off].any() and not got[:, :, 1][off].any(), (what, "a flow where valid is 0")
    both = ((got_valid == 1) & (wvalid == 1))[:, :, None]
    return check_values(got, want, bound, what, mask=np.broadcast_to(both, got.shape))


# ---- the cases, run the same way on the emulation and on the device ----------------------------------------------------------
def image_case(lib, H, W, h, w, V, B, C, form, device="cpu"):
    """One pf_viewport_image case against the statement; returns (output, worst ratio or half-integer share)."""
    rows, t32 = rows_of(V, h, w)
    what = f"image {form} {H}x{W} -> {V} x {h}x{w}, B={B} C={C} on {device}"
    seed = H + 3 * h + V + B
    if form == "f32":
        x = make_image(B, C, H, W, seed)
        got = run_image(lib, x, t32, device)
        return got, check_values(got, vr.view_image(x, t32), image_bound(x, t32), what)
    x = make_u8(B, C, H, W, seed)
    got = run_image(lib, x, t32, device)
    val, _ = vr.view_image_u8(x, t32)
    bound = image_bound(x.transpose(0, 3, 1, 2), t32).transpose(0, 1, 3, 4, 2)
    return got, check_bytes(got, val, bound, what)


def flow_case(lib, H, W, h, w, V, kind, device="cpu"):
    rows, t32 = rows_of(V, h, w)
    B = 2 if kind in ("smooth", "smooth_nan") else 1
    flow = make_flow(kind, B, H, W, seed=V)
    got, valid = run_flow(lib, flow, t32, MIN_FORWARD, device)
    worst = check_flow(got, valid, flow, t32, f"flow {kind} {H}x{W} -> {V} x {h}x{w}, B={B} on {device}")
    return got, valid, worst


def cube_case(lib, s, H, W, B, C, device="cpu"):
    faces = make_faces(B, C, s, seed=s + B)
    got = run_cube(lib, faces, H, W, device)
    return got, check_values(got, vr.cubemap_to_erp(faces, H, W), cube_bound(faces, H, W), f"cube {s} -> {H}x{W}, B={B} C={C} on {device}")
