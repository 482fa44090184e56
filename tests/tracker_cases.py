"""Seeded pair scenes and runners shared by tests/test_tracker_host.py (the host emulation) and tests/test_hip_tracker.py (the
device): the emulation's handle, a tracker driven through the typed wrappers on numpy inputs, the sweep of shapes, table sizes,
directions and pair families, and a four-frame version of the analytic moving-ball scene.  Not collected.

The ids, counts and sums of every scene come from tests/segments_ref.py (flood fill), never from the code under test."""
import ctypes
import functools
import math

import numpy as np
import torch

import segments_cases as sc
import segments_ref as sr
import tracker_ref as tr
from prior_flow_amd.object_tracks import ObjectTracker
from prior_flow_amd.segments import MovingObjects

ENTRIES = sc.ENTRIES + ("pf_trk_begin", "pf_trk_vote", "pf_trk_match", "pf_trk_paint")
# (B, H, W): one pixel, smaller than a wave, odd sizes with two images, W = 64 k +- 1, more than one row of waves, rows longer
# than a workgroup
SHAPES = ((1, 1, 1), (1, 2, 3), (2, 17, 37), (1, 33, 70), (2, 64, 128), (1, 130, 257), (1, 40, 1100))
# (max_objects, min_area): a table that overflows (count > M), the LDS path's largest table, the global-atomic path
SETTINGS = ((8, 0.0), (64, 1.5), (200, 0.0))
DIRECTIONS = ("forward", "backward", "both")
FAMILIES = ("static", "shift", "seam", "swap", "split", "tie", "merge", "birth_death", "masked", "junk", "bernoulli_0.41",
            "bernoulli_0.5")
MIN_OVERLAP = 0.25
# The paths that exist only on the device (tests/launch_paths.py), kept apart from SHAPES: (B, H, W), B = sc.TWO_PER_CU standing for
# twice the card's CU count.
#   (2 cus, 24, 48)    24 items against a cap of ONE workgroup of 16 waves: a second trip in which half the waves have nothing
#   (2, 512, 1024)     the product size: 512 workgroups wanted against a cap of `cus`
DEVICE_PATHS = ((sc.TWO_PER_CU, 24, 48), (2, 512, 1024))
FULL_TABLE = (256, 0.0)                          # PF_TRK_MAX_OBJECTS: every thread of the match kernel owns a slot
DEVICE_SETTINGS = SETTINGS + (FULL_TABLE,)
DEVICE_FAMILIES = ("shift", "seam", "split", "junk", "bernoulli_0.41")
OVERFLOWS = ((2, 512, 1024), "bernoulli_0.41")   # more than 256 objects in both frames
DISTINCT = 8                                     # a large batch repeats its first DISTINCT images: image b is image b % DISTINCT
INT_KEYS = ("votes", "track", "age", "origin", "fate", "next_id", "track_map")
STATE_KEYS = ("st_ids", "st_count", "st_sums", "st_track", "st_age", "st_path")


@functools.lru_cache(maxsize=None)
def emu():
    """PfLib handle of tests/emu/libpf_emu_tracker.so (built on demand): the tracker's and the segments' entry points."""
    import __graft_entry__ as ge
    from prior_flow_amd import _lib
    so = ge.build_emu_tracker()
    lib = _lib.PfLib(so, require_cuda=False, optional=tuple(n for n in _lib.EXPORTS if n not in ENTRIES))
    lib._dll.pf_emu_trk_order.argtypes = [ctypes.c_ulonglong]
    lib._dll.pf_emu_trk_order.restype = None
    return lib


# ---- pair scenes ---------------------------------------------------------------------------------------------------------------
def _box(m, y0, x0, h, w):
    """Sets rows y0..y0+h (clipped) and columns x0..x0+w (cyclic) of m; -> the boolean map of what it set."""
    H, W = m.shape
    on = np.zeros((H, W), bool)
    ys = np.arange(max(y0, 0), min(y0 + max(h, 1), H))
    xs = np.arange(x0, x0 + max(w, 1)) % W
    on[np.ix_(ys, xs)] = True
    m[on] = 1
    return on


def _noise(rng, H, W):
    return rng.uniform(-0.39, 0.39, (2, H, W))                          # below 0.4 px: the nearest pixel stays the planted one


def _wrap(u, W):
    return (u + W / 2) % W - W / 2                                        # into [-W/2, W/2)


def _image(family, H, W, rng):
    """(mask0, mask1, forward flow on frame 0's grid, backward flow on frame 1's grid, occ0 or None, occ1 or None) of one image."""
    m0, m1 = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    fw, bw = _noise(rng, H, W), _noise(rng, H, W)
    occ0 = occ1 = None
    hA, wA, hB, wB = max(H // 5, 1), max(W // 8, 1), max(H // 6, 1), max(W // 10, 1)
    pA, pB = (H // 4, W // 8), (H // 2, (5 * W) // 8)
    if family.startswith("bernoulli_"):
        m0[:] = rng.random((H, W)) < float(family.split("_")[1])
        m1[:] = np.roll(m0, 2, axis=1)
        y, x = np.mgrid[0:H, 0:W]
        f1, f2 = rng.uniform(0, 2 * np.pi, 2)
        smooth = np.stack([2 + 0.8 * np.sin(2 * np.pi * y / H + f1), 0.8 * np.cos(2 * np.pi * x / W + f2)])
        fw, bw = fw + smooth, bw - smooth
    elif family in ("static", "shift", "seam", "masked", "junk"):
        dx, dy = {"static": (0, 0), "seam": (5, 0)}.get(family, (3, 1) if H > 8 and W > 12 else (1, 0))
        a = _box(m0, pA[0], W - 3 - wA if family == "seam" else pA[1], hA, wA)          # seam: ends 3 columns before the seam, moves 5
        _box(m0, pB[0], pB[1], hB, wB)
        m1[:] = np.roll(m0, (dy, dx), axis=(0, 1))
        fw[0] += _wrap(dx, W)
        fw[1] += dy
        bw[0] += _wrap(-dx, W)
        bw[1] -= dy
        if family == "static":
            fw[:], bw[:] = 0, 0
        if family == "masked":                                            # an occlusion byte over the left half of the first object
            occ0 = np.zeros((H, W), np.uint8)
            occ0[a & (np.arange(W)[None, :] < pA[1] + (wA + 1) // 2)] = 1
            occ1 = np.roll(occ0, (dy, dx), axis=(0, 1))
        if family == "junk":
            vals = np.array([np.nan, np.inf, -np.inf, 2.0 ** 30, -2.0 ** 30, H + 5.0, -(H + 5.0)])
            for f in (fw, bw):
                hit = rng.random((H, W)) < 0.03
                pick = rng.integers(0, len(vals), int(hit.sum()))
                ch = np.where(pick >= 5, 1, rng.integers(0, 2, int(hit.sum())))       # v beyond either pole: channel 1
                f[ch, np.nonzero(hit)[0], np.nonzero(hit)[1]] = vals[pick]
    elif family == "swap":
        a, b = _box(m0, *pA, hA, wA), _box(m0, *pB, hB, wB)
        a1, b1 = _box(m1, *pB, hA, wA), _box(m1, *pA, hB, wB)             # frame 1: the shapes have changed places
        d = (pB[1] - pA[1], pB[0] - pA[0])
        for k in (0, 1):
            fw[k][a] += d[k]
            fw[k][b] -= d[k]
            bw[k][a1] -= d[k]
            bw[k][b1] += d[k]
    elif family in ("split", "tie", "merge"):
        half = max(W // 6, 1)
        # tie: two equal pieces; else a piece of a fifth of the bar, below a quarter of it: min and max of the areas part ways
        L, cut = (2 * half + 1, half) if family == "tie" else (max(W // 3, 3), max(W // 3, 3) // 5)
        whole, parts = (m1, m0) if family == "merge" else (m0, m1)
        _box(whole, H // 3, W // 4, hB, L)
        _box(parts, H // 3, W // 4, hB, cut)                                # the bar without its column `cut`
        if L - cut - 1 > 0:
            _box(parts, H // 3, W // 4 + cut + 1, hB, L - cut - 1)
        fw[:], bw[:] = 0, 0
    elif family == "birth_death":
        _box(m0, *pA, hA, wA)
        _box(m0, *pB, hB, wB)                                               # dies
        _box(m1, *pA, hA, wA)
        _box(m1, (3 * H) // 4, W // 3, hB, wB)                              # is born
        fw[:], bw[:] = 0, 0
    return m0, m1, fw.astype(np.float32), bw.astype(np.float32), occ0, occ1


@functools.lru_cache(maxsize=None)
def pair(family, B, H, W, seed=0):
    """dict(masks (mask0, mask1) uint8 [B,H,W], fw, bw fp32 [B,2,H,W], occ (occ0, occ1) uint8 [B,H,W] or None, labels (lab0, lab1)
    by flood fill at 8-connectivity)."""
    imgs = [_image(family, H, W, np.random.default_rng([seed, b, H, W, FAMILIES.index(family)])) for b in range(B)]
    stack = lambda k: np.stack([im[k] for im in imgs])                    # noqa: E731
    occ = (stack(4), stack(5)) if imgs[0][4] is not None else None
    masks = (stack(0), stack(1))
    return dict(masks=masks, fw=stack(2), bw=stack(3), occ=occ, labels=tuple(sr.labels(m, 8, False) for m in masks))


def objects(lab, rows, cols, M, min_area):
    """ids, count, sums of labels [B,H,W] under the given tables (tests/segments_ref.py)."""
    o = sr.objects(lab, rows, cols, None, M, min_area)
    return o["ids"], o["count"], o["sums"]


def flows(p, direction):
    """(flow_prev, flow_cur, mask_prev, mask_cur) of a pair under one of DIRECTIONS."""
    occ = p["occ"] or (None, None)
    f, g = direction in ("forward", "both"), direction in ("backward", "both")
    return (p["fw"] if f else None, p["bw"] if g else None, occ[0] if f else None, occ[1] if g else None)


def device_case(case, cus=256):
    """(B, H, W) of one of DEVICE_PATHS on a card of `cus` CUs."""
    return (2 * cus if case[0] == sc.TWO_PER_CU else case[0],) + tuple(case[1:])


def tiled(a, B):
    """An array (or each array of a tuple or dict) over the distinct images, repeated to B images: image b is image b % K."""
    if isinstance(a, dict):
        return {k: tiled(v, B) for k, v in a.items()}
    if isinstance(a, tuple):
        return tuple(tiled(v, B) for v in a)
    return None if a is None else np.ascontiguousarray(np.asarray(a)[np.arange(B) % len(a)])


@functools.lru_cache(maxsize=None)
def device_pair(family, B, H, W):
    """(pair of the min(B, DISTINCT) distinct images, the same repeated to B images): the flood fill runs once per distinct image."""
    small = pair(family, min(B, DISTINCT), H, W)
    return small, (small if B <= DISTINCT else tiled(small, B))


def run_pair_tiled(lib, small, full, obj0, obj1, rows, direction, M, device="cpu"):
    """run_pair on a batch that repeats its distinct images, beside the reference's pushes of the distinct images alone (obj0, obj1:
    their objects), repeated: -> run_pair's four.  The reference continues the code's own path of the distinct images."""
    B, K = full["masks"][0].shape[0], small["masks"][0].shape[0]
    H, W = obj0[0].shape[1:]
    g1, g2 = run_pair(lib, full, tiled(obj0, B), tiled(obj1, B), rows, direction, M, device, ref=False)
    r1 = tr.push(tr.empty_state(K, H, W, M), *obj0, np.zeros((K, 2, H, W), np.float32), None, None, None, rows, MIN_OVERLAP)
    assert sc.bits(g1["st_path"]).tolist() == sc.bits(tiled(g1["st_path"][:K], B)).tolist(), "the repeats of an image differ"
    r2 = tr.push(dict(r1[1], path=g1["st_path"][:K]), *obj1, *flows(small, direction), rows, MIN_OVERLAP)
    return g1, g2, tiled(r1, B), tiled(r2, B)


# ---- runners -------------------------------------------------------------------------------------------------------------------
class Tracker:
    """The four entry points on numpy inputs, with the state kept on `device`.  offset = 1: every pixel map lives one element into
    its buffer; poison: the outputs and the vote matrix start as 0xFF bytes / NaN."""

    def __init__(self, lib, B, H, W, M, device="cpu", offset=0, poison=False):
        self.lib, self.shape, self.M, self.device, self.offset, self.poison = lib, (B, H, W), M, device, offset, poison
        z = lambda shape, dt, off=0: sc._blank(shape, dt, device, off)     # noqa: E731
        self.st_ids, self.st_count = z((B, H, W), torch.int32, offset), z((B,), torch.int32)
        self.st_sums = z((B, M, tr.SUMS), torch.int64)
        self.st_track, self.st_age, self.st_path = z((B, M), torch.int32), z((B, M), torch.int32), z((B, M), torch.float32)
        self.next_id = sc._blank((B,), torch.int32, device, 0, 1)

    def push(self, ids, count, sums, flow_prev, flow_cur, mask_prev, mask_cur, rows, min_overlap=MIN_OVERLAP):
        (B, H, W), M, dev, off = self.shape, self.M, self.device, self.offset
        fill = -1 if self.poison else 0
        up = lambda a, o=0: None if a is None else sc._shifted(a, dev, o)  # noqa: E731
        t_ids, t_count, t_sums, t_rows = up(ids, off), up(np.asarray(count, np.int32)), up(sums), up(rows)
        t_fp, t_fc, t_mp, t_mc = up(flow_prev, off), up(flow_cur, off), up(mask_prev, off), up(mask_cur, off)
        votes = sc._blank((B, M, M), torch.int64, dev, 0, fill)
        i32 = lambda: sc._blank((B, M), torch.int32, dev, 0, fill)         # noqa: E731
        f32 = lambda: sc._blank((B, M), torch.float32, dev, 0, float("nan") if self.poison else 0.0)  # noqa: E731
        track, age, origin, fate, step, path = i32(), i32(), i32(), i32(), f32(), f32()
        track_map = sc._blank((B, H, W), torch.int32, dev, off, fill)
        lib = self.lib
        lib.trk_begin(votes)
        lib.trk_vote(self.st_ids, t_ids, t_fp, t_fc, t_mp, t_mc, t_rows, votes)
        lib.trk_match(votes, t_count, t_sums, self.st_count, self.st_sums, self.st_track, self.st_age, self.st_path, self.next_id, track,
                      age, origin, fate, step, path, (flow_prev is not None) + (flow_cur is not None), min_overlap)
        lib.trk_paint(t_ids, track, track_map, self.st_ids)
        if dev != "cpu":
            torch.cuda.synchronize()
        out = dict(votes=votes, track=track, age=age, origin=origin, fate=fate, step=step, path=path, track_map=track_map,
                   next_id=self.next_id, st_ids=self.st_ids, st_count=self.st_count, st_sums=self.st_sums, st_track=self.st_track,
                   st_age=self.st_age, st_path=self.st_path)
        return {k: t.cpu().numpy().copy() for k, t in out.items()}

    def state(self):
        """The state as tests/tracker_ref.py's dict (the code's own path)."""
        g = lambda t: t.cpu().numpy().copy()                               # noqa: E731
        return dict(ids=g(self.st_ids), count=g(self.st_count), sums=g(self.st_sums), track=g(self.st_track), age=g(self.st_age),
                    path=g(self.st_path), next_id=g(self.next_id))


def same_bits(a, b, what):
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, f"{what}: {k}"
        bad = sc.bits(a[k]) != sc.bits(b[k])
        assert not bad.any(), f"{what}: {k} differs in {int(bad.sum())} of {bad.size} cells, first at {np.argwhere(bad)[0].tolist()}"


def against_reference(got, ref, nxt, what, scale=1.0):
    """Every integer bit for bit (the state the push left included); step and path within scale x the reference's bound.
    -> the worst error / bound."""
    want = dict(ref, st_ids=nxt["ids"], st_count=nxt["count"], st_sums=nxt["sums"], st_track=nxt["track"], st_age=nxt["age"])
    for k in INT_KEYS + STATE_KEYS[:-1]:
        assert got[k].dtype == want[k].dtype, f"{what}: {k} is {got[k].dtype}"
        bad = got[k] != want[k]
        assert not bad.any(), f"{what}: {k} differs in {int(bad.sum())} of {bad.size} cells, first at {np.argwhere(bad)[0].tolist()}"
    assert sc.bits(got["st_path"]).tolist() == sc.bits(got["path"]).tolist(), f"{what}: the kept path is not the path"
    worst = 0.0
    for k in ("step", "path"):
        assert np.isfinite(got[k]).all(), f"{what}: {k} is not finite"
        d, bound = np.abs(got[k].astype(np.float64) - ref[k]), scale * ref[k + "_bound"]
        assert (d <= bound).all(), f"{what}: {k} off by {d.max():.3e}, bound {bound[np.unravel_index(d.argmax(), d.shape)]:.3e}"
        worst = max(worst, float(np.where(bound > 0, d / np.where(bound > 0, bound, 1), 0).max()))
    return worst


def within_bound(got, want, what, scale=2.0):
    """step and path of two runs of the code (the device's and the emulation's) within scale x the reference's bound, which is
    evaluated at `want`: each may be off by one bound.  -> the worst difference / (scale x bound)."""
    step_b = tr.U * np.abs(want["step"].astype(np.float64)) + 2.0 ** -48
    path_b = (1 + tr.U) * step_b + tr.U * np.abs(want["path"].astype(np.float64))
    worst = 0.0
    for k, bound in (("step", step_b), ("path", path_b)):
        assert np.isfinite(got[k]).all(), f"{what}: {k} is not finite"
        d = np.abs(got[k].astype(np.float64) - want[k].astype(np.float64))
        assert (d <= scale * bound).all(), f"{what}: {k} off by {d.max():.3e}"
        worst = max(worst, float((d / (scale * bound)).max()))
    return worst


def run_pair(lib, p, obj0, obj1, rows, direction, M, device="cpu", fault=None, ref=True, **kw):
    """Two pushes through the entry points (the first makes every object new, the second links the pair) beside the reference's:
    -> (got of push 1, got of push 2, (ref, next) of push 1, (ref, next) of push 2); ref = False: the first two alone."""
    B, H, W = obj0[0].shape
    t = Tracker(lib, B, H, W, M, device, **kw)
    link = flows(p, direction)
    zero = np.zeros((B, 2, H, W), np.float32)
    g1 = t.push(*obj0, zero, None, None, None, rows)
    if not ref:
        return g1, t.push(*obj1, *link, rows)
    r1 = tr.push(tr.empty_state(B, H, W, M), *obj0, zero, None, None, None, rows, MIN_OVERLAP, fault)
    state = dict(r1[1], path=g1["st_path"])
    g2 = t.push(*obj1, *link, rows)
    r2 = tr.push(state, *obj1, *link, rows, MIN_OVERLAP, fault)
    return g1, g2, r1, r2


# ---- the moving ball over four frames -------------------------------------------------------------------------------------------
BALL_FRAMES = 4
BALL_SPECKLE = 0.003
# path against three times the planted step, relatively.  The path sums the lengths of three centroid steps of s = |(1.5, -0.75)|
# = 1.68 px.  With e_k the centroid's quantisation error in frame k, the errors along the motion telescope to e_3 - e_0 and those
# across it enter each step's length only in second order (e^2 / 2 s).  sc.ball_check allows a centroid one pixel off per axis for a
# SINGLE frame against the analytic centre; between two frames of the same disc moved by a fraction of a pixel most of that is
# common to both and cancels, and a tenth of the path (0.5 px over the 5 px of three steps, a quarter of a pixel per end) is what is
# asked of the difference.
BALL_PATH_TOL = 0.10


def ball_sequence(H, W, theta, seed=0):
    """Four frames of a ball (a disc of angular radius sc.BALL['radius']) whose centre advances by sc.BALL['motion'] pixels per
    frame before a static background, seen by a static camera, with isolated speckle of the same motion.  -> dict(moving [K] uint8
    [1,H,W] on each pair's first frame, fw, bw [K] fp32 [1,2,H,W], inv_depth, steps: the K - 1 planted great-circle steps)."""
    rng = np.random.default_rng([seed, H, W, 26])
    P, x, y = sc._sphere(H, W)
    mx, my = sc.BALL["motion"]
    c0 = np.array([math.cos(sc.BALL["phi"]) * math.cos(theta), math.cos(sc.BALL["phi"]) * math.sin(theta), math.sin(sc.BALL["phi"])])
    cx0, cy0 = sc._erp(c0, H, W)

    def centre(k):
        th, ph = ((cx0 + k * mx + 0.5) / W - 0.5) * 2 * np.pi, (0.5 - (cy0 + k * my + 0.5) / H) * np.pi
        return np.array([math.cos(ph) * math.cos(th), math.cos(ph) * math.sin(th), math.sin(ph)])

    balls = [np.arccos(np.clip(P @ centre(k), -1, 1)) <= sc.BALL["radius"] for k in range(BALL_FRAMES + 1)]
    moving, fws, bws, last = [], [], [], None
    for k in range(BALL_FRAMES):
        grown = balls[k].copy()
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                grown |= np.roll(np.roll(balls[k], dy, 0), dx, 1)
        speck = (rng.random((H, W)) < BALL_SPECKLE) & ~grown
        if k > 0:                                                          # speckle is new every frame: none where the last frame's lies or lands
            for dy in (-2, -1, 0, 1):
                for dx in (-1, 0, 1, 2, 3):
                    speck &= ~np.roll(np.roll(last, dy, 0), dx, 1)
        last = speck
        fw, bw = 0.05 * rng.standard_normal((2, H, W)), 0.05 * rng.standard_normal((2, H, W))
        fw[0][balls[k] | speck] += mx
        fw[1][balls[k] | speck] += my
        bw[0][balls[k + 1]] -= mx
        bw[1][balls[k + 1]] -= my
        moving.append((np.hypot(*fw) > sc.BALL["thr"]).astype(np.uint8)[None])
        fws.append(fw[None].astype(np.float32))
        bws.append(bw[None].astype(np.float32))
    steps = [math.acos(min(1.0, float(centre(k) @ centre(k + 1)))) for k in range(BALL_FRAMES - 1)]
    inv_depth = np.where(balls[0], sc.BALL["inv_depth"], sc.BALL["wall"])[None].astype(np.float32)
    return dict(moving=moving, fw=fws, bw=bws, inv_depth=inv_depth, steps=steps)


def ball_track(seq, H, W, device, lib=None):
    """The sequence through MovingObjects.update + ObjectTracker.push (grid = "first") -> per frame (track, age, path, pixels, count)
    as numpy arrays."""
    from collections import namedtuple
    mo = MovingObjects(1, H, W, device, min_area=0.5, lib=lib)
    tk = ObjectTracker(mo, grid="first")
    R = namedtuple("R", "forward backward occ_forward occ_backward")
    out = []
    for k in range(BALL_FRAMES):
        dev = lambda a: torch.from_numpy(a).to(device)                     # noqa: E731
        mo.update(dev(seq["moving"][k]))
        track, age, _ = tk.push(R(dev(seq["fw"][k]), dev(seq["bw"][k]), None, None))
        out.append(tuple(t.cpu().numpy().copy() for t in (track, age, tk.path, mo.sums[..., 1], mo.count)))
    return out


def ball_track_check(frames, seq, what):
    """One track id for the ball (the object with the most pixels) over all four frames, age 4, the path within BALL_PATH_TOL of
    three times the planted step, no other track older than 1.  Prints the figures."""
    ids, path = [], 0.0
    for k, (track, age, pth, pixels, count) in enumerate(frames):
        n = min(int(count[0]), track.shape[1])
        assert n >= 1, f"{what}: no object in frame {k}"
        ball = int(np.argmax(pixels[0, :n]))
        ids.append(int(track[0, ball]))
        assert int(age[0, ball]) == k + 1, f"{what}: the ball's age in frame {k} is {int(age[0, ball])}"
        others = np.delete(age[0, :n], ball)
        assert (others <= 1).all(), f"{what}: a speckle track of age {int(others.max())} in frame {k}"
        path = float(pth[0, ball])
    want = 3 * seq["steps"][0]
    print(f"[tracker] {what}: ball track ids {ids}, path {path:.5f} rad against 3 x planted step {want:.5f} rad "
          f"({100 * (path / want - 1):+.2f} %), sum of the three planted steps {sum(seq['steps']):.5f}")
    assert len(set(ids)) == 1 and ids[0] >= 1, f"{what}: the ball's track ids are {ids}"
    assert abs(path - want) <= BALL_PATH_TOL * want, f"{what}: path {path:.5f} against {want:.5f}"
