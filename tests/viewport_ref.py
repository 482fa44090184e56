"""Float64 numpy statement of the perspective viewports and cube maps, written from the definition and
not from the kernel.  Not collected; imported by tests/test_viewport_host.py and tests/test_hip_viewport.py.

ERP pixel (m, n) of an H x W map: theta = ((m + 1/2) / W - 1/2) 2 pi, phi = (1/2 - (n + 1/2) / H) pi,
s(m, n) = (cos phi cos theta, cos phi sin theta, sin phi); a direction d lies at theta = atan2(d_y, d_x), phi = asin(d_z / |d|),
m = (theta / 2 pi + 1/2) W - 1/2, n = (1/2 - phi / pi) H - 1/2 (no diverge_zero nudge).  A view is (R, f, h, w) with R's columns
forward, right, up, principal point ((w - 1) / 2, (h - 1) / 2), camera ray (1, (j - c_x) / f, -(i - c_y) / f) of pixel (i, j),
world ray d = R ray, proj(q) = (c_x + f q_r / q_f, c_y - f q_u / q_f), (q_f, q_r, q_u) = R^T q.

Every function takes `fault`: None, or the name of one deliberate mistake (FAULTS) that tests/test_viewport_host.py builds into a
copy of the statement to show that the cases notice it.
"""
import numpy as np

FAULTS = ("principal_point", "x_not_wrapped", "y_not_clamped", "roll_sign", "r_transposed", "u_interpolated",
          "endpoint_not_clamped", "up_down_swapped", "tie_order", "valid_before_sum")

# columns [forward, right, up] of the six faces: front, right, back, left, up, down
CUBE = (((1, 0, 0), (0, 1, 0), (0, 0, 1)), ((0, 1, 0), (-1, 0, 0), (0, 0, 1)), ((-1, 0, 0), (0, -1, 0), (0, 0, 1)),
        ((0, -1, 0), (1, 0, 0), (0, 0, 1)), ((0, 0, 1), (0, 1, 0), (-1, 0, 0)), ((0, 0, -1), (0, 1, 0), (1, 0, 0)))


def rotation(yaw, pitch, roll, fault=None):
    """Rz(yaw) Ry(pitch) Rx(roll): generate_rotation_metrix(theta_list=[yaw, pitch, roll])."""
    if fault == "roll_sign":
        roll = -roll
    cz, sz, cy, sy, cx, sx = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]])
    ry = np.array([[cy, 0, sy], [0, 1.0, 0], [-sy, 0, cy]])
    rx = np.array([[1.0, 0, 0], [0, cx, -sx], [0, sx, cx]])
    return rz @ ry @ rx


def viewport_row(yaw, pitch, roll, fov_x_deg, h, w, fault=None):
    """One row {R row-major, f, h, w} of a view table, float64."""
    f = (w / 2.0) / np.tan(np.radians(fov_x_deg) / 2.0)
    return np.concatenate([rotation(yaw, pitch, roll, fault).reshape(-1), [f, h, w]])


def cube_rows(s, fault=None):
    faces = list(CUBE)
    if fault == "up_down_swapped":
        faces[4], faces[5] = faces[5], faces[4]
    return np.array([np.concatenate([np.array(c, np.float64).T.reshape(-1), [s / 2.0, s, s]]) for c in faces])


def table32(rows):
    """The table as the C-ABI takes it: fp32.  The statement is evaluated on these values (widened back), so that the rounding of
    the inputs is no part of the error."""
    return np.ascontiguousarray(np.asarray(rows, np.float64).reshape(-1, 12).astype(np.float32))


def sphere(m, n, H, W):
    theta = ((np.asarray(m, np.float64) + 0.5) / W - 0.5) * 2 * np.pi
    phi = (0.5 - (np.asarray(n, np.float64) + 0.5) / H) * np.pi
    return np.stack(np.broadcast_arrays(np.cos(phi) * np.cos(theta), np.cos(phi) * np.sin(theta), np.sin(phi)), -1)


def erp_of(d, H, W):
    d = np.asarray(d, np.float64)
    theta = np.arctan2(d[..., 1], d[..., 0])
    phi = np.arcsin(np.clip(d[..., 2] / np.linalg.norm(d, axis=-1), -1, 1))
    return (theta / (2 * np.pi) + 0.5) * W - 0.5, (0.5 - phi / np.pi) * H - 0.5


def _view(row, fault=None):
    row = np.asarray(row, np.float64)
    R, f, h, w = row[:9].reshape(3, 3), row[9], int(row[10]), int(row[11])
    if fault == "r_transposed":
        R = R.T
    cx, cy = ((w / 2.0, h / 2.0) if fault == "principal_point" else ((w - 1) / 2.0, (h - 1) / 2.0))
    return R, f, h, w, cx, cy


def rays(row, fault=None):
    """World rays d [h,w,3] of a view's pixels."""
    R, f, h, w, cx, cy = _view(row, fault)
    i, j = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    cam = np.stack([np.ones_like(i), (j - cx) / f, -(i - cy) / f], -1)
    return cam @ R.T


def proj(q, row, fault=None):
    R, f, h, w, cx, cy = _view(row, fault)
    c = np.asarray(q, np.float64) @ R                       # R^T q
    with np.errstate(divide="ignore", invalid="ignore"):
        return cx + f * c[..., 1] / c[..., 0], cy - f * c[..., 2] / c[..., 0], c[..., 0]


def wraptaps(m, n, H, W, fault=None):
    """The model's cyclic taps (core/utils/my_cycle_sample.py:31-60): x wraps, y clamps, weights from the unclamped fraction.
    -> (rows [4,...], columns [4,...], weights [4,...], zero mask [4,...]) in the order (y0,x0), (y1,x0), (y0,x1), (y1,x1)."""
    m = np.asarray(m, np.float64)
    n = np.asarray(n, np.float64)
    if fault != "x_not_wrapped":
        m = np.mod(m, W)
    x0, y0 = np.floor(m), np.floor(n)
    xw, yw = m - x0, n - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    x1, y1 = x0 + 1, y0 + 1
    if fault == "x_not_wrapped":
        x0, x1 = np.clip(x0, 0, W - 1), np.clip(x1, 0, W - 1)
    else:
        x0, x1 = x0 % W, x1 % W
    dead = [np.zeros(m.shape, bool)] * 4
    if fault == "y_not_clamped":                            # rows past the border read as zero instead of the border row
        dead = [(y0 < 0) | (y0 > H - 1), (y1 < 0) | (y1 > H - 1)] * 2
    y0, y1 = np.clip(y0, 0, H - 1), np.clip(y1, 0, H - 1)
    ys = np.stack([y0, y1, y0, y1])
    xs = np.stack([x0, x0, x1, x1])
    ws = np.stack([(1 - xw) * (1 - yw), (1 - xw) * yw, xw * (1 - yw), xw * yw])
    return ys, xs, ws, np.stack(dead)


def view_positions(rows, H, W, fault=None):
    """(m, n) [V,h,w] of every view pixel's ray."""
    mn = [erp_of(rays(r, fault), H, W) for r in rows]
    return np.stack([a for a, _ in mn]), np.stack([b for _, b in mn])


def view_image(x, rows, fault=None):
    """ERP [B,C,H,W] -> views [B,V,C,h,w], float64."""
    x = np.asarray(x, np.float64)
    B, C, H, W = x.shape
    m, n = view_positions(rows, H, W, fault)
    ys, xs, ws, dead = wraptaps(m, n, H, W, fault)
    taps = x[:, :, ys, xs]                                   # [B,C,4,V,h,w]
    taps = np.where(dead[None, None], 0.0, taps)
    return (taps * ws[None, None]).sum(2).transpose(0, 2, 1, 3, 4)


def view_image_u8(x, rows, fault=None):
    """uint8 [B,H,W,C] -> (the float64 value before rounding [B,V,h,w,C], floor(x + 1/2) clamped to 0..255)."""
    val = view_image(np.asarray(x, np.float64).transpose(0, 3, 1, 2), rows, fault).transpose(0, 1, 3, 4, 2)
    return val, np.clip(np.floor(val + 0.5), 0, 255).astype(np.uint8)


def displacement(flow, fault=None):
    """D [B,H,W,3] = e - s of every ERP pixel: s = s(m, n), e = s(m + u, clamp(n + v, -1/2, H - 1/2)) (flow2endpoint's rule)."""
    flow = np.asarray(flow, np.float64)
    B, _, H, W = flow.shape
    n, m = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    en = n + flow[:, 1]
    if fault != "endpoint_not_clamped":
        en = np.clip(en, -0.5, H - 0.5)
    with np.errstate(invalid="ignore"):
        return sphere(m + flow[:, 0], en, H, W) - sphere(m, n, H, W)[None]


def view_flow(flow, rows, min_forward, fault=None):
    """ERP flow [B,2,H,W] -> (pinhole flow [B,V,2,h,w], valid uint8 [B,V,h,w], cosine q_f / |q| [B,V,h,w]), float64."""
    flow = np.asarray(flow, np.float64)
    B, _, H, W = flow.shape
    finite = np.isfinite(flow).all(1)                        # [B,H,W]
    D = displacement(np.where(finite[:, None], flow, 0.0), fault)
    out, valid, cosine = [], [], []
    for r in rows:
        d = rays(r, fault)
        p = d / np.linalg.norm(d, axis=-1, keepdims=True)
        m, n = erp_of(d, H, W)
        ys, xs, ws, dead = wraptaps(m, n, H, W, fault)
        ok = finite[:, ys, xs].all(1)                        # [B,h,w]
        if fault == "u_interpolated":                        # the flow itself blended, then one end point from (m, n)
            f4 = np.where(dead[None, None], 0.0, np.where(finite[:, None], flow, 0.0)[:, :, ys, xs])
            uv = (f4 * ws[None, None]).sum(2)                # [B,2,h,w]
            q = p[None] + sphere(m[None] + uv[:, 0], np.clip(n[None] + uv[:, 1], -0.5, H - 0.5), H, W) - sphere(m, n, H, W)[None]
        else:
            taps = np.where(dead[None, ..., None], 0.0, D[:, ys, xs])          # [B,4,h,w,3]
            q = p[None] + (taps * ws[None, ..., None]).sum(1)
        qx, qy, qf = proj(q, r, fault)
        px, py, pf = proj(p, r, fault)
        cq = qf / np.linalg.norm(q, axis=-1)
        front = (np.broadcast_to(pf / np.linalg.norm(p, axis=-1), cq.shape) if fault == "valid_before_sum" else cq) > min_forward
        ok = ok & front
        with np.errstate(invalid="ignore"):
            o = np.stack([np.where(ok, qx - px[None], 0.0), np.where(ok, qy - py[None], 0.0)], 1)
        out.append(np.nan_to_num(o, nan=0.0, posinf=0.0, neginf=0.0) if fault == "valid_before_sum" else o)
        valid.append(ok.astype(np.uint8))
        cosine.append(cq)
    return np.stack(out, 1), np.stack(valid, 1), np.stack(cosine, 1)


def cube_face(d, fault=None):
    """Face index of directions d [...,3]: the axis with the largest |component|, ties to the earlier face."""
    d = np.asarray(d, np.float64)
    fwd = np.stack([d[..., 0], d[..., 1], -d[..., 0], -d[..., 1], d[..., 2], -d[..., 2]], -1)
    if fault == "tie_order":
        return 5 - np.argmax(fwd[..., ::-1], -1)
    return np.argmax(fwd, -1)                                # argmax returns the first maximum


def cube_positions(s, H, W, fault=None):
    """(face, x, y) [H,W] of every ERP pixel's direction on its face."""
    n, m = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    d = sphere(m, n, H, W)
    face = cube_face(d, fault)
    rows = cube_rows(s, fault)
    px, py = np.zeros((H, W)), np.zeros((H, W))
    for k in range(6):
        x, y, _ = proj(d, rows[k])
        px, py = np.where(face == k, x, px), np.where(face == k, y, py)
    return face, px, py


def cubemap_to_erp(faces, H, W, fault=None):
    """Cube faces [B,6,C,s,s] -> ERP [B,C,H,W], float64: bilinear with the taps clamped to the face."""
    faces = np.asarray(faces, np.float64)
    s = faces.shape[-1]
    face, px, py = cube_positions(s, H, W, fault)
    x0, y0 = np.floor(px), np.floor(py)
    xw, yw = px - x0, py - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    c = lambda a: np.clip(a, 0, s - 1)                      # noqa: E731
    g = lambda yy, xx: faces[:, face, :, c(yy), c(xx)]      # noqa: E731  [H,W,B,C] (advanced indices first)
    out = (g(y0, x0) * ((1 - xw) * (1 - yw))[..., None, None] + g(y0 + 1, x0) * ((1 - xw) * yw)[..., None, None]
           + g(y0, x0 + 1) * (xw * (1 - yw))[..., None, None] + g(y0 + 1, x0 + 1) * (xw * yw)[..., None, None])
    return out.transpose(2, 3, 0, 1)


def yaw_flow_closed_form(rows, alpha):
    """The pinhole flow [V,2,h,w] of the rigid yaw rotation by alpha that a constant-u ERP flow u = alpha W / (2 pi) encodes:
    every direction turns about the z axis, d -> Rz(alpha) d, and is projected back."""
    rz = rotation(alpha, 0.0, 0.0)
    out = []
    for r in rows:
        d = rays(r)
        p = d / np.linalg.norm(d, axis=-1, keepdims=True)
        qx, qy, _ = proj(p @ rz.T, r)
        px, py, _ = proj(p, r)
        out.append(np.stack([qx - px, qy - py]))
    return np.stack(out)
