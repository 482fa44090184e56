"""Plain Python / numpy statement of the connected components of a mask on the cyclic panorama, their integer sums and the object
table, written from the definition and not from the header: a breadth-first flood fill over the
neighbourhood, no union-find, no tiles.  Not collected; imported by tests/test_segments_host.py and tests/test_hip_segments.py.

Every function takes `fault`: None, or the name of one deliberate mistake (FAULTS) that tests/test_segments_host.py builds into a
copy of the statement to show that the cases notice it.

The integer sums are built from the fp32 tables the caller hands over (the device's own, read back), with numpy's fp32 products:
one IEEE rounding each, as in the header, so every sum is compared bit for bit.  The table is evaluated in float64 from those
integers.  The bounds on the fp32 table (U = 2^-24):
  area, pixels, resultant, value weight, means: the code under test evaluates them in fp64 from the same integers and rounds once
    to fp32; its fp64 operations (a few products, one square root, one quotient) are off by 2^-53 relatively, which disappears
    beside the rounding to fp32: |error| <= 2 U |value|.
  centroid: the summed bearing is normalised in fp64 and cast to fp32 (each component relatively U: an angle of at most 2 U), then
    pf_vp_erp in fp32: hypot (two products, a sum, a root: 2 U relatively, an angle of at most 2 U in phi), atan2f (at most 4 ulp
    of a value up to pi: 4 * 2 U * pi < 26 U), in all ANGLE = 32 U; then (angle / 2 pi + 1/2) W - 1/2 in four roundings of values up
    to W: 4 U W.  x: W (ANGLE / 2 pi + 4 U), compared cyclically (theta = +-pi is one direction); y: H (ANGLE / pi + 4 U).
"""
import collections
import math

import numpy as np

FAULTS = ("no_seam", "no_seam_diagonal", "no_corner_diagonal", "max_label", "four_for_eight", "area_no_cos", "ids_off_by_one",
          "count_clipped", "poles_ignored", "nan_counted")
U = 2.0 ** -24
ANGLE = 32 * U
SUMS, COLS = 10, 6
F, FV, VMAX = 2.0 ** 32, 2.0 ** 16, 65536.0
TILE_H, TILE_W = 32, 64          # only the planted fault no_corner_diagonal knows about tiles


def neighbours(y, x, H, W, conn, fault=None):
    """The linear indices of the pixels (y, x) touches (background or not)."""
    if fault == "four_for_eight":
        conn = 4
    steps = ((0, -1), (0, 1), (-1, 0), (1, 0)) + (((-1, -1), (-1, 1), (1, -1), (1, 1)) if conn == 8 else ())
    out = []
    for dy, dx in steps:
        yy, xx = y + dy, x + dx
        if yy < 0 or yy >= H:
            continue                                                     # rows do not wrap
        wrapped = xx < 0 or xx >= W
        xx %= W
        if wrapped and (fault == "no_seam" or (dy != 0 and fault == "no_seam_diagonal")):
            continue
        if fault == "no_corner_diagonal" and dy != 0 and dx != 0 and not wrapped and xx // TILE_W != x // TILE_W \
                and yy // TILE_H != y // TILE_H:
            continue
        out.append(yy * W + xx)
    return out


def label_image(mask, conn, poles, fault=None):
    """labels int32 [H,W] of one mask [H,W]: 1 + the smallest linear index of the component, 0 for background."""
    H, W = mask.shape
    flat = (np.asarray(mask).reshape(-1) != 0).tolist()
    lab = [0] * (H * W)
    seen = [False] * (H * W)
    pole_rows = sorted({0, H - 1}) if poles and fault != "poles_ignored" else []
    members = {r: [r * W + x for x in range(W) if flat[r * W + x]] for r in pole_rows}
    for start in range(H * W):
        if not flat[start] or seen[start]:
            continue
        comp, queue = [], collections.deque([start])
        seen[start] = True
        joined = set()
        while queue:
            i = queue.popleft()
            comp.append(i)
            y, x = divmod(i, W)
            near = neighbours(y, x, H, W, conn, fault)
            if y in members and y not in joined:                         # the pixels of a pole row meet at the pole
                joined.add(y)
                near = near + members[y]
            for j in near:
                if flat[j] and not seen[j]:
                    seen[j] = True
                    queue.append(j)
        label = 1 + (max(comp) if fault == "max_label" else min(comp))
        for i in comp:
            lab[i] = label
    return np.array(lab, np.int32).reshape(H, W)


def labels(mask, conn, poles, fault=None):
    return np.stack([label_image(m, conn, poles, fault) for m in mask])


def _quant(v, scale):
    """pf_ego_quant of an fp32 array: llrintf(v * scale), the product exact for a power of two."""
    return np.rint((v.astype(np.float32) * np.float32(scale)).astype(np.float64)).astype(np.int64)


def pixel_sums(rows, cols, values, b, fault=None):
    """int64 [SUMS,H,W]: what each pixel of image b adds to its object."""
    rows, cols = np.asarray(rows, np.float32), np.asarray(cols, np.float32)
    H, W = rows.shape[0], cols.shape[0]
    cp = np.broadcast_to(rows[:, 0:1], (H, W)).astype(np.float32)
    sp = np.broadcast_to(rows[:, 1:2], (H, W)).astype(np.float32)
    ct = np.broadcast_to(cols[None, :, 0], (H, W)).astype(np.float32)
    st = np.broadcast_to(cols[None, :, 1], (H, W)).astype(np.float32)
    px, py, pz = cp * ct, cp * st, sp                                   # fp32 products, one rounding each
    s = np.zeros((SUMS, H, W), np.int64)
    s[0] = _quant(np.ones_like(cp) if fault == "area_no_cos" else cp, F)
    s[1] = 1
    s[2], s[3], s[4] = _quant(cp * px, F), _quant(cp * py, F), _quant(cp * pz, F)
    if values is not None:
        v = np.asarray(values[b], np.float32)
        with np.errstate(invalid="ignore"):
            ok = ~(np.abs(v) >= VMAX).any(0) if fault == "nan_counted" else (np.abs(v) < VMAX).all(0)
        v = np.where(np.isnan(v), np.float32(0), v) if fault == "nan_counted" else v
        s[5] = np.where(ok, s[0], 0)
        for c in range(v.shape[0]):
            with np.errstate(invalid="ignore", over="ignore"):
                s[6 + c] = np.where(ok, _quant(np.where(ok, cp * v[c], np.float32(0)), FV), 0)
    return s


def objects(lab, rows, cols, values, M, min_area, fault=None):
    """dict(ids, keep, roots, count, sums, table (float64), bound) of labels [B,H,W]."""
    B, H, W = lab.shape
    C = 0 if values is None else values.shape[1]
    min_q = math.ceil(float(np.float32(min_area)) * F)
    ids, keep = np.zeros((B, H, W), np.int32), np.zeros((B, H, W), np.uint8)
    roots, count = np.full((B, M), -1, np.int32), np.zeros(B, np.int32)
    sums, table = np.zeros((B, M, SUMS), np.int64), np.zeros((B, M, COLS + C), np.float64)
    bound = np.zeros((B, M, COLS + C), np.float64)
    for b in range(B):
        ps = pixel_sums(rows, cols, values, b, fault).reshape(SUMS, -1)
        flat = lab[b].reshape(-1)
        at = np.nonzero(flat)[0]
        comps, inv = np.unique(flat[at], return_inverse=True)                 # ascending: by the root's linear index
        cs = np.zeros((len(comps), SUMS), np.int64)
        np.add.at(cs, inv, ps[:, at].T)                                       # integer adds: exact
        surv = cs[:, 0] >= min_q
        rank = np.cumsum(surv) * surv                                         # 1, 2, ... over the survivors, 0 elsewhere
        count[b] = min(int(surv.sum()), M) if fault == "count_clipped" else int(surv.sum())
        r = rank[inv]
        keep[b].reshape(-1)[at] = r > 0
        shown = (r > 0) & (r <= M)
        ids[b].reshape(-1)[at] = np.where(shown, r - 1 if fault == "ids_off_by_one" else r, 0)
        for k, c in enumerate(np.nonzero(surv)[0][:M]):
            roots[b, k] = comps[c] - 1
            sums[b, k] = cs[c]
            table[b, k], bound[b, k] = resolve(cs[c], C, H, W)
    return dict(ids=ids, keep=keep, roots=roots, count=count, sums=sums, table=table, bound=bound)


def resolve(s, C, H, W):
    """(row, bound) of one object's table, float64, from its integer sums."""
    s = [int(v) for v in s]
    t, e = np.zeros(COLS + C), np.zeros(COLS + C)
    t[0], t[1] = s[0] / F, s[1]
    if s[2] or s[3] or s[4]:
        bx, by, bz = s[2] / F, s[3] / F, s[4] / F
        theta, phi = math.atan2(by, bx), math.atan2(bz, math.hypot(bx, by))
        t[2] = (theta / (2 * math.pi) + 0.5) * W - 0.5
        t[3] = (0.5 - phi / math.pi) * H - 0.5
        t[4] = math.sqrt(bx * bx + by * by + bz * bz) / t[0] if s[0] > 0 else 0.0
    t[5] = s[5] / F
    for c in range(C):
        t[COLS + c] = (s[6 + c] / FV) / t[5] if s[5] > 0 else 0.0
    e[:] = 2 * U * np.abs(t) + 1e-30
    e[2] = W * (ANGLE / (2 * math.pi) + 4 * U)
    e[3] = H * (ANGLE / math.pi + 4 * U)
    return t, e


def table_error(got, want, bound, W):
    """The worst |got - want| / bound over a table; the centroid's x is compared cyclically."""
    d = np.abs(np.asarray(got, np.float64) - want)
    d[..., 2] = np.minimum(d[..., 2], np.abs(W - d[..., 2]))
    ratio = np.where(bound > 0, d / np.where(bound > 0, bound, 1.0), np.where(d == 0, 0.0, np.inf))     # an unused row is exactly zero
    return float(ratio.max()) if d.size else 0.0
