"""Plain Python / numpy statement of the object tracks, written from the definition and not from the header:
the votes by ``np.add.at`` in int64, the threshold, the match and the bookkeeping in loops, the step from exact integer cross and
dot products.  Not collected; imported by tests/test_tracker_host.py and tests/test_hip_tracker.py.

Every function takes `fault`: None, or the name of one deliberate mistake (FAULTS) that tests/test_tracker_host.py builds into a
copy of the statement to show that the cases notice it.

The integers (votes, track, age, origin, fate, next_id, track_map) are compared bit for bit.  The bounds on step and path
(U = 2^-24, u = 2^-53):
  step: the code under test converts the six 64-bit sums to fp64 (relative u each: the two vectors turn by at most 2 u each), forms
    the cross product in fp64 (two products and a difference per component: at most 3 u |p| |c| each, 5.2 u |p| |c| in the norm,
    plus 3 u relatively for the squares, their sum and the root) and the dot product (at most 5 u |p| |c|); atan2(n, d) moves by at
    most (|dn| + |dd|) / (|p| |c|) because n^2 + d^2 = |p|^2 |c|^2, and is itself good to a few u of a value up to pi.  In all
    less than 2^-49 radians, absolutely.  This file forms both products exactly in Python integers, so its own error is the root's
    and atan2's, a few u relatively.  The result is rounded once to fp32: U |step|.   bound = U |step| + 2^-48.
  path: fp32(previous path) + fp32(step), one fp32 add: the step's error, then U of the sum.  The previous path is the code's own
    (the caller hands it over), so nothing accumulates.                                bound = (1 + U) bound(step) + U |path|.
"""
import math

import numpy as np

FAULTS = ("no_wrap", "truncate", "mask_ignored", "no_transpose", "ties_largest", "row_only", "thr_max", "ids_top_down", "age_stuck",
          "merged_lost")
U = 2.0 ** -24
SUMS = 10
F = 2.0 ** 32
FAR = 2.0 ** 30


def _quant(v, scale):
    """pf_ego_quant of an fp32 array: llrintf(v * scale), the product exact for a power of two."""
    return np.rint((np.asarray(v, np.float32) * np.float32(scale)).astype(np.float64)).astype(np.int64)


def empty_state(B, H, W, M):
    return dict(ids=np.zeros((B, H, W), np.int32), count=np.zeros(B, np.int32), sums=np.zeros((B, M, SUMS), np.int64),
                track=np.zeros((B, M), np.int32), age=np.zeros((B, M), np.int32), path=np.zeros((B, M), np.float32),
                next_id=np.ones(B, np.int32))


def _direction(S, src, dst, flow, mask, rows, M, transposed, fault):
    """The votes of one flow: src, dst int32 [B,H,W], flow fp32 [B,2,H,W], mask uint8 [B,H,W] or None, into S int64 [B,M,M]."""
    B, H, W = src.shape
    x = np.broadcast_to(np.arange(W, dtype=np.float32)[None, :], (H, W))
    y = np.broadcast_to(np.arange(H, dtype=np.float32)[:, None], (H, W))
    q = np.broadcast_to(_quant(np.asarray(rows, np.float32)[:, 0], F)[:, None], (H, W))
    half = np.float32(0.5)
    for b in range(B):
        u, v = np.asarray(flow[b, 0], np.float32), np.asarray(flow[b, 1], np.float32)
        with np.errstate(invalid="ignore"):
            ok = (np.abs(u) < FAR) & (np.abs(v) < FAR)                     # a NaN compares false
        if mask is not None and fault != "mask_ignored":
            ok &= np.asarray(mask[b]) == 0
        u, v = np.where(ok, u, np.float32(0)), np.where(ok, v, np.float32(0))
        if fault == "truncate":
            xt, yt = np.trunc(x + u), np.trunc(y + v)
        else:
            xt, yt = np.floor((x + u) + half), np.floor((y + v) + half)    # fp32 adds, one rounding each
        xt, yt = xt.astype(np.int64), yt.astype(np.int64)
        ok &= (yt >= 0) & (yt < H)
        if fault == "no_wrap":
            ok &= (xt >= 0) & (xt < W)
        xt %= W
        s = src[b].astype(np.int64)
        ok &= (s > 0) & (s <= M)
        d = dst[b][np.clip(yt, 0, H - 1), xt].astype(np.int64)
        ok &= (d > 0) & (d <= M)
        a, c = (d, s) if transposed and fault != "no_transpose" else (s, d)
        np.add.at(S[b], (a[ok] - 1, c[ok] - 1), q[ok])


def votes(prev_ids, ids, flow_prev, flow_cur, mask_prev, mask_cur, rows, M, fault=None):
    """S int64 [B,M,M]: flow_prev lives on the previous grid and points into the current frame, flow_cur the other way."""
    S = np.zeros((prev_ids.shape[0], M, M), np.int64)
    if flow_prev is not None:
        _direction(S, prev_ids, ids, flow_prev, mask_prev, rows, M, False, fault)
    if flow_cur is not None:
        _direction(S, ids, prev_ids, flow_cur, mask_cur, rows, M, True, fault)
    return S


def _best(values, fault):
    """The smallest index of the largest positive value, -1 when there is none."""
    top = max(values, default=0)
    if top <= 0:
        return -1
    at = [i for i, v in enumerate(values) if v == top]
    return at[-1] if fault == "ties_largest" else at[0]


def step_angle(p, c):
    """(angle in float64, bound) between two summed bearings given as three integers each."""
    p, c = [int(v) for v in p], [int(v) for v in c]
    if not any(p) or not any(c):
        return 0.0, 0.0
    k = (p[1] * c[2] - p[2] * c[1], p[2] * c[0] - p[0] * c[2], p[0] * c[1] - p[1] * c[0])          # exact
    n2, d = sum(v * v for v in k), sum(a * b for a, b in zip(p, c))
    ang = math.atan2(math.sqrt(n2), d)
    return ang, U * abs(ang) + 2.0 ** -48


def match(state, count, sums, S, n_dir, min_overlap, fault=None):
    """One push without its pixel maps: -> dict(track, age, origin, fate int32 [B,M]; step, path float64 [B,M] with step_bound,
    path_bound; next_id int32 [B]).  state: the previous frame's dict (empty_state's keys); state['path'] is the code's own."""
    B, M = S.shape[:2]
    mo = float(np.float32(min_overlap))
    out = dict(track=np.zeros((B, M), np.int32), age=np.zeros((B, M), np.int32), origin=np.zeros((B, M), np.int32),
               fate=np.zeros((B, M), np.int32), step=np.zeros((B, M)), path=np.zeros((B, M)), step_bound=np.zeros((B, M)),
               path_bound=np.zeros((B, M)), next_id=np.zeros(B, np.int32))
    for b in range(B):
        n_p, n_c = max(0, min(int(state["count"][b]), M)), max(0, min(int(count[b]), M))
        Ap, Ac = [int(v) for v in state["sums"][b, :, 0]], [int(v) for v in sums[b, :, 0]]
        E = [[0] * n_c for _ in range(n_p)]
        for a in range(n_p):
            for c in range(n_c):
                small = max(Ap[a], Ac[c]) if fault == "thr_max" else min(Ap[a], Ac[c])
                thr = math.ceil(mo * float(n_dir * small))
                s = int(S[b, a, c])
                E[a][c] = s if s >= max(1, thr) else 0
        rowbest = [_best(E[a], fault) for a in range(n_p)]
        colbest = [_best([E[a][c] for a in range(n_p)], fault) for c in range(n_c)]
        if fault == "row_only":
            cont = [next((a for a in range(n_p) if rowbest[a] == c), -1) for c in range(n_c)]
        else:
            cont = [colbest[c] if colbest[c] >= 0 and rowbest[colbest[c]] == c else -1 for c in range(n_c)]
        fresh = [c for c in range(n_c) if cont[c] < 0]
        nxt = int(state["next_id"][b])
        for c in range(n_c):
            a = cont[c]
            if a >= 0:
                trk = int(state["track"][b, a])
                out["track"][b, c], out["origin"][b, c] = trk, trk
                out["age"][b, c] = int(state["age"][b, a]) + (0 if fault == "age_stuck" else 1)
                ang, e = step_angle(state["sums"][b, a, 2:5], sums[b, c, 2:5])
                out["step"][b, c], out["step_bound"][b, c] = ang, e
                out["path"][b, c] = float(state["path"][b, a]) + ang
                out["path_bound"][b, c] = (1 + U) * e + U * abs(out["path"][b, c])
            else:
                below = sum(1 for f in fresh if (f > c if fault == "ids_top_down" else f < c))
                out["track"][b, c], out["age"][b, c] = nxt + below, 1
                out["origin"][b, c] = int(state["track"][b, colbest[c]]) if colbest[c] >= 0 else 0
        for a in range(n_p):
            r = rowbest[a]
            if r >= 0:
                out["fate"][b, a] = r + 1 if cont[r] == a else (0 if fault == "merged_lost" else -(r + 1))
        out["next_id"][b] = nxt + len(fresh)
    return out


def push(state, ids, count, sums, flow_prev, flow_cur, mask_prev, mask_cur, rows, min_overlap=0.25, fault=None):
    """One whole push: -> (outputs, the next state).  outputs: match's keys, votes and track_map.  The next state's path is the
    float64 one rounded to fp32; a caller that checks a sequence replaces it by the code's own."""
    B, M = sums.shape[:2]
    S = votes(state["ids"], ids, flow_prev, flow_cur, mask_prev, mask_cur, rows, M, fault)
    out = match(state, count, sums, S, (flow_prev is not None) + (flow_cur is not None), min_overlap, fault)
    out["votes"] = S
    tm = np.zeros_like(ids)
    for b in range(B):
        on = (ids[b] > 0) & (ids[b] <= M)
        tm[b][on] = out["track"][b][ids[b][on] - 1]
    out["track_map"] = tm
    nxt = dict(ids=ids.copy(), count=np.asarray(count, np.int32).copy(), sums=sums.copy(), track=out["track"].copy(), age=out["age"].copy(),
               path=out["path"].astype(np.float32), next_id=out["next_id"].copy())
    return out, nxt
