"""Seeded masks and runners shared by tests/test_segments_host.py (the host emulation) and tests/test_hip_segments.py (the device):
the emulation's handle, a whole update through the typed wrappers on numpy inputs, the sweep of shapes and mask families and the
analytic moving-ball scene.  Not collected."""
import ctypes
import functools
import math

import numpy as np
import torch

import segments_ref as sr

ENTRIES = ("pf_seg_scratch_bytes", "pf_seg_tables", "pf_seg_label", "pf_seg_objects")
# (B, C, H, W): a tile smaller than a wave, W = 64 k +- 1, ragged tiles on both axes, more than two tiles each way, rows longer than
# a workgroup; C = 0..4 all occur
SWEEP = ((1, 0, 1, 1), (1, 1, 2, 3), (1, 3, 6, 10), (2, 4, 17, 37), (3, 0, 24, 48), (1, 2, 33, 70), (2, 3, 64, 128), (1, 1, 130, 257),
         (1, 4, 40, 1100))
BERNOULLI = (0.3, 0.41, 0.5, 0.59, 0.7)          # both site-percolation thresholds (0.593 at 4, 0.407 at 8) lie inside
FAMILIES = ("empty", "full", "checker", "vstripes", "hstripes", "serpentine", "spiral", "seam_blob", "corner_diag", "seam_diag",
            "pole_scatter", "junk") + tuple(f"bernoulli_{p}" for p in BERNOULLI)
POLE_FAMILIES = ("empty", "checker", "hstripes", "pole_scatter", "bernoulli_0.41")
# (connectivity, poles, max_objects, min_area) of the sweep: a small table that overflows with every component kept, the defaults,
# and a table beyond what the accumulate kernel keeps in LDS (512)
SETTINGS = ((4, False, 8, 0.0), (8, False, 64, 1.5), (8, True, 64, 1.5), (4, True, 600, 0.0))

# The paths that exist only on the device (tests/launch_paths.py), kept apart from SWEEP: (B, C, H, W), with B = TWO_PER_CU standing
# for twice the card's CU count (512 on a whole MI355X, and for the host twin).
#   (2 cus, 1, 24, 48)   the accumulate grid is capped at ONE workgroup per image: a full first trip and a second of 128 pixels
#   (2, 3, 512, 1024)    the product size with both directions: 512 workgroups wanted against a cap of `cus`; the scan holds 2 rows
#   (1, 1, 257, 66)      the scan holds 2 rows per thread, thread 128 holds one, the threads from 129 none; W = 64 + 2
#   (1, 0, 600, 8)       3 rows per thread, the threads from 200 hold none; a map narrower than a wave
TWO_PER_CU = "2cus"
DEVICE_PATHS = ((TWO_PER_CU, 1, 24, 48), (2, 3, 512, 1024), (1, 1, 257, 66), (1, 0, 600, 8))
# ... at the sweep's settings and at the two tables at their limits: the largest kept in LDS and PF_SEG_MAX_OBJECTS
FULL_TABLES = ((8, False, 512, 0.0), (4, False, 4096, 0.0))
DEVICE_SETTINGS = SETTINGS + FULL_TABLES
DEVICE_FAMILIES = ("full", "serpentine", "hstripes", "junk", "bernoulli_0.41", "bernoulli_0.59")
# where both new tables overflow (54 204 and 7 401 survivors per image against 4096 and 512 rows)
OVERFLOWS = ((2, 3, 512, 1024), "bernoulli_0.41")
ORDERS = (1, 2, 77, 123456789)                   # pf_emu_seg_order: reversed, and three shuffles


def device_case(case, cus=256):
    """(B, C, H, W) of one of DEVICE_PATHS on a card of `cus` CUs."""
    return (2 * cus if case[0] == TWO_PER_CU else case[0],) + tuple(case[1:])


def case_id(case):
    return "x".join(str(n) for n in case)


def device_combos(family):
    """The settings a family of DEVICE_FAMILIES runs at: the pole settings apply to the horizontal stripes alone."""
    return tuple(s for s in DEVICE_SETTINGS if not s[1] or family == "hstripes")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


@functools.lru_cache(maxsize=None)
def emu():
    """PfLib handle of tests/emu/libpf_emu_segments.so (built on demand)."""
    import __graft_entry__ as ge
    from prior_flow_amd import _lib
    so = ge.build_emu_segments()
    lib = _lib.PfLib(so, require_cuda=False, optional=tuple(n for n in _lib.EXPORTS if n not in ENTRIES))
    lib._dll.pf_emu_seg_order.argtypes = [ctypes.c_ulonglong]
    lib._dll.pf_emu_seg_order.restype = None
    return lib


def combos(family):
    """The settings a family runs at: both connectivities, poles where they matter."""
    return tuple(s for s in SETTINGS if not s[1] or family in POLE_FAMILIES)


# ---- masks -------------------------------------------------------------------------------------------------------------------
def _image(family, H, W, rng):
    m = np.zeros((H, W), np.uint8)
    y, x = np.mgrid[0:H, 0:W]
    if family == "full":
        m[:] = 1
    elif family == "checker":
        m[:] = (x + y) % 2 == 0
    elif family == "vstripes":
        m[:] = x % 2 == 0                       # every stripe crosses every horizontal tile border
    elif family == "hstripes":
        m[:] = y % 2 == 0                       # every stripe crosses every vertical tile border and the seam
    elif family == "serpentine":
        # one snake: the even rows without their last column (so the seam is no shortcut), joined at alternating ends
        m[0::2, :max(W - 1, 1)] = 1
        for r in range(1, H - 1, 2):
            m[r, max(W - 2, 0) if (r // 2) % 2 == 0 else 0] = 1
    elif family == "spiral":
        # a walker that turns right whenever the cell two ahead is taken or outside; the last column stays clear
        Ws = max(W - 1, 1)
        cy, cx, d = 0, 0, 0
        m[0, 0] = 1
        step = ((0, 1), (1, 0), (0, -1), (-1, 0))
        turns = 0
        while turns < 2:
            dy, dx = step[d]
            ny, nx, ay, ax = cy + dy, cx + dx, cy + 2 * dy, cx + 2 * dx
            free = 0 <= ny < H and 0 <= nx < Ws and not m[ny, nx] and not (0 <= ay < H and 0 <= ax < Ws and m[ay, ax])
            if free:
                cy, cx, turns = ny, nx, 0
                m[cy, cx] = 1
            else:
                d, turns = (d + 1) % 4, turns + 1
    elif family == "seam_blob":
        m[H // 3:H // 3 + max(H // 4, 1), :min(2, W)] = 1
        m[H // 3:H // 3 + max(H // 4, 1), max(W - 3, 0):] = 1
    elif family == "corner_diag":
        # two blobs that touch only diagonally, across the tile corner (32, 64) where the image has one
        cy, cx = (32, 64) if H > 34 and W > 66 else (max(H // 2, 1), max(W // 2, 1))
        m[max(cy - 2, 0):cy, max(cx - 2, 0):cx] = 1
        m[cy:cy + 2, cx:cx + 2] = 1
        if H > 70 and W > 130:                  # and the other diagonal at the next corner
            m[62:64, 128:130] = 1
            m[64:66, 126:128] = 1
    elif family == "seam_diag":
        r = H // 2
        m[max(r - 1, 0):r + 1, max(W - 2, 0):] = 1                            # ends in (W-1, r)
        if r + 1 < H:
            m[r + 1:r + 3, :min(2, max(W - 3, 1))] = 1                        # starts in (0, r+1)
    elif family == "pole_scatter":
        m[0] = rng.random(W) < 0.3
        m[H - 1] = rng.random(W) < 0.3
        m[:] |= (rng.random((H, W)) < 0.02).astype(np.uint8)
    elif family == "junk":
        m[:] = rng.choice(np.array([0, 0, 2, 255], np.uint8), size=(H, W))
    elif family.startswith("bernoulli_"):
        m[:] = rng.random((H, W)) < float(family.split("_")[1])
    return m


@functools.lru_cache(maxsize=None)
def mask(family, B, H, W, seed=0):
    """uint8 [B,H,W]: image b of a drawn family has its own seed, of a fixed one is shifted by 7 b columns."""
    out = []
    for b in range(B):
        rng = np.random.default_rng([seed, b, H, W, FAMILIES.index(family)])
        out.append(np.roll(_image(family, H, W, rng), 7 * b, axis=1))
    m = np.stack(out)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def values(B, C, H, W, seed=0):
    """fp32 [B,C,H,W] or None: a smooth field plus noise, with NaN, infinities and values at and beyond 2^16 sprinkled in."""
    if C == 0:
        return None
    rng = np.random.default_rng([seed, B, C, H, W])
    v = (10 * rng.standard_normal((B, C, H, W))).astype(np.float32)
    junk = np.array([np.nan, np.inf, -np.inf, 65536.0, -65536.0, 1e30, 65535.996], np.float32)
    hit = rng.random((B, C, H, W)) < 0.03
    v[hit] = rng.choice(junk, size=int(hit.sum()))
    v.setflags(write=False)
    return v


# ---- runners -----------------------------------------------------------------------------------------------------------------
KEYS = ("labels", "ids", "keep", "roots", "count", "sums", "table")


def _shifted(a, device, offset, dtype=None):
    """`a` on the device in a buffer that starts `offset` elements early (offset = 1: an unaligned map)."""
    t = torch.from_numpy(np.array(a))
    buf = torch.zeros(t.numel() + offset, dtype=t.dtype, device=device)
    view = buf[offset:].view(t.shape)
    view.copy_(t)
    return view


def _blank(shape, dtype, device, offset, fill=0):
    n = int(np.prod(shape))
    buf = torch.full((n + offset,), fill, dtype=dtype, device=device)
    return buf[offset:].view(shape)


def tables(lib, H, W, device="cpu"):
    """(rows [H,2], cols [W,2]) fp32 as this library computes them, as numpy arrays."""
    rows = torch.zeros(H, 2, dtype=torch.float32, device=device)
    cols = torch.zeros(W, 2, dtype=torch.float32, device=device)
    lib.seg_tables(rows, cols)
    return rows.cpu().numpy(), cols.cpu().numpy()


def run(lib, m, v, conn, poles, M, min_area, device="cpu", offset=0, tabs=None, poison=False):
    """One update through the entry points: dict of numpy arrays (KEYS, rows, cols).  tabs: the tables to use instead of the
    library's own (the device's, for the emulation); poison: every output and the scratch start as 0xFF bytes."""
    B, H, W = m.shape
    C = 0 if v is None else v.shape[1]
    rows, cols = tabs if tabs is not None else tables(lib, H, W, device)
    fill = -1 if poison else 0
    tm, tv = _shifted(m, device, offset), None if v is None else _shifted(v, device, offset)
    trows, tcols = _shifted(rows, device, 0), _shifted(cols, device, 0)
    scratch = torch.full((lib.seg_scratch_bytes(B, H, W) // 8,), fill, dtype=torch.int64, device=device)
    labels, ids = _blank((B, H, W), torch.int32, device, offset, fill), _blank((B, H, W), torch.int32, device, offset, fill)
    keep = _blank((B, H, W), torch.uint8, device, offset, 255 if poison else 0)
    roots, count = _blank((B, M), torch.int32, device, 0, fill), _blank((B,), torch.int32, device, 0, fill)
    table = _blank((B, M, sr.COLS + C), torch.float32, device, 0, float("nan") if poison else 0.0)
    sums = _blank((B, M, sr.SUMS), torch.int64, device, 0, fill)
    lib.seg_label(tm, trows, labels, scratch, conn, poles)
    lib.seg_objects(labels, tv, trows, tcols, scratch, ids, keep, roots, count, table, sums, min_area)
    if device != "cpu":
        torch.cuda.synchronize()
    out = dict(labels=labels, ids=ids, keep=keep, roots=roots, count=count, sums=sums, table=table)
    out = {k: t.cpu().numpy().copy() for k, t in out.items()}
    out["rows"], out["cols"] = rows, cols
    return out


def same_bits(a, b, what):
    for k in KEYS:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, f"{what}: {k}"
        bad = bits(a[k]) != bits(b[k])
        assert not bad.any(), f"{what}: {k} differs in {int(bad.sum())} of {bad.size} cells, first at {np.argwhere(bad)[0].tolist()}"


@functools.lru_cache(maxsize=None)
def flood_fill(family, B, H, W, conn, poles):
    """tests/segments_ref.py's labels of mask(family, B, H, W), once per connectivity: they do not depend on the table's size."""
    lab = sr.labels(mask(family, B, H, W), conn, poles)
    lab.setflags(write=False)
    return lab


def reference(m, v, conn, poles, M, min_area, rows, cols, fault=None, lab=None):
    lab = sr.labels(m, conn, poles, fault) if lab is None else lab
    out = sr.objects(lab, rows, cols, v, M, min_area, fault)
    out["labels"] = lab
    return out


def against_reference(got, ref, what):
    """Everything integer bit for bit; the table within the reference's bound.  -> worst error / bound."""
    for k in ("labels", "ids", "keep", "roots", "count", "sums"):
        assert got[k].dtype == ref[k].dtype, f"{what}: {k} is {got[k].dtype}"
        bad = got[k] != ref[k]
        assert not bad.any(), f"{what}: {k} differs in {int(bad.sum())} of {bad.size} cells, first at {np.argwhere(bad)[0].tolist()}"
    assert np.isfinite(got["table"]).all(), f"{what}: the table is not finite"
    worst = sr.table_error(got["table"], ref["table"], ref["bound"], got["labels"].shape[2])
    assert worst <= 1.0, f"{what}: table error / bound = {worst:.3f}"
    return worst


# ---- the analytic moving-ball scene ------------------------------------------------------------------------------------------
def _sphere(H, W):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    th, ph = ((x + 0.5) / W - 0.5) * 2 * np.pi, (0.5 - (y + 0.5) / H) * np.pi
    return np.stack([np.cos(ph) * np.cos(th), np.cos(ph) * np.sin(th), np.sin(ph)], -1), x, y


def _erp(X, H, W):
    th, ph = np.arctan2(X[..., 1], X[..., 0]), np.arctan2(X[..., 2], np.hypot(X[..., 0], X[..., 1]))
    return (th / (2 * np.pi) + 0.5) * W - 0.5, (0.5 - ph / np.pi) * H - 0.5


# (H, W, theta of the ball's centre): the second ball straddles the seam
BALL_SCENES = ((32, 64, 0.7), (64, 128, math.pi - 0.04))
BALL = dict(phi=0.3, radius=0.3, motion=(1.5, -0.75), inv_depth=0.5, wall=0.25, speckle=0.01, thr=0.5)


def ball_scene(H, W, theta, seed=0):
    """A static wall at inverse depth 0.25 seen from a camera that turns and moves, and a ball (a disc of angular radius 0.3 on the
    sphere at inverse depth 0.5) that moves by itself: on top of the rigid flow its pixels carry the planted motion.  One percent
    of the other pixels are isolated outliers of the same size (speckle).  -> dict(moving, flow, rigid_flow, inv_depth, centre
    (x, y) in ERP pixels, motion); moving = |flow - rigid_flow| > 0.5 px, which is what a residual threshold gives."""
    rng = np.random.default_rng([seed, H, W])
    P, x, y = _sphere(H, W)
    a = 0.02
    R = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])
    T = np.array([0.05, 0.02, -0.01])
    c = np.array([math.cos(BALL["phi"]) * math.cos(theta), math.cos(BALL["phi"]) * math.sin(theta), math.sin(BALL["phi"])])
    ball = np.arccos(np.clip(P @ c, -1, 1)) <= BALL["radius"]
    d = np.where(ball, BALL["inv_depth"], BALL["wall"])
    qx, qy = _erp(P @ R.T + d[..., None] * T, H, W)
    rigid = np.stack([np.mod(qx - x + W / 2, W) - W / 2, qy - y])
    speck = (rng.random((H, W)) < BALL["speckle"]) & ~ball
    grown = ball.copy()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            grown |= np.roll(np.roll(ball, dy, 0), dx, 1)
    speck &= ~grown                                                     # no speckle that touches the ball
    own = np.zeros((2, H, W))
    own[0][ball | speck], own[1][ball | speck] = BALL["motion"]
    flow = rigid + own + 0.05 * rng.standard_normal((2, H, W))
    moving = (np.hypot(*(flow - rigid)) > BALL["thr"]).astype(np.uint8)
    cx, cy = _erp(c, H, W)
    return dict(moving=moving[None], flow=flow[None].astype(np.float32), rigid_flow=rigid[None].astype(np.float32),
                inv_depth=d[None].astype(np.float32), centre=(float(cx), float(cy)), motion=BALL["motion"], pixels=int(ball.sum()))


def ball_check(table, count, scene, W, what):
    """The largest object is the ball: its centroid within one pixel of the ball's centre, its mean independent motion of the
    planted sign and within a factor two of the planted size, its mean inverse depth the ball's.  Prints the figures."""
    n = min(int(count[0]), table.shape[1])
    assert n >= 1, f"{what}: no object"
    k = int(np.argmax(table[0, :n, 0]))
    area, pixels, cx, cy, res, vw, mu, mv, md = (float(t) for t in table[0, k, :9])
    ex = abs(cx - scene["centre"][0])
    ex, ey = min(ex, W - ex), abs(cy - scene["centre"][1])
    print(f"[segments] {what}: {int(count[0])} objects; ball {int(pixels)} px (planted {scene['pixels']}), area {area:.1f}, centroid off by "
          f"({ex:.3f}, {ey:.3f}) px, resultant {res:.4f}, mean motion ({mu:.3f}, {mv:.3f}) planted {scene['motion']}, mean 1/depth {md:.3f}")
    assert ex <= 1.0 and ey <= 1.0
    for got, want in ((mu, scene["motion"][0]), (mv, scene["motion"][1])):
        assert got * want > 0 and 0.5 * abs(want) <= abs(got) <= 2 * abs(want)
    assert abs(md - BALL["inv_depth"]) <= 0.05 and abs(pixels - scene["pixels"]) <= 0.05 * scene["pixels"] and res > 0.9
