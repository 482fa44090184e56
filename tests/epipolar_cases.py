"""Seeded scenes and runners shared by tests/test_epipolar_host.py (the host emulation) and tests/test_hip_epipolar.py (the device):
the emulation's handle, one estimate / pass / map through the typed wrappers on numpy inputs, and the checks that hold a result
to the float64 restatement (tests/epipolar_ref.py)."""
import ctypes
import functools

import numpy as np
import torch

import egomotion_cases as ec
import egomotion_ref as er
import epipolar_ref as pr

SHAPES = ec.SHAPES
TRANSLATIONS = ((0.3, -0.2, 0.93), (0, 1, 0), (-1, 0, 0))
BASELINES = (0.1, 0.3)
ENTRIES = ("pf_ego_scratch_bytes", "pf_ego_accumulate", "pf_ego_solve", "pf_epi_sums_bytes", "pf_epi_accumulate", "pf_epi_solve",
           "pf_epi_map")
MOVING_CAP = 0.02                  # the share of `moving` bytes that may lie within the bound of a threshold


@functools.lru_cache(maxsize=None)
def emu():
    """PfLib handle of tests/emu/libpf_emu_epipolar.so (built on demand): the epipolar entry points and the two of the rotation
    estimate a PoseEstimator needs."""
    import __graft_entry__ as ge
    from prior_flow_amd import _lib
    so = ge.build_emu_epipolar()
    lib = _lib.PfLib(so, require_cuda=False, optional=tuple(n for n in _lib.EXPORTS if n not in ENTRIES))
    lib._dll.pf_emu_epi_order.argtypes = [ctypes.c_ulonglong]
    lib._dll.pf_emu_epi_order.restype = None
    lib._dll.pf_emu_epi_worst.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_longlong)]
    lib._dll.pf_emu_epi_worst.restype = None
    return lib


_t = ec._t


# ---- scenes ----------------------------------------------------------------------------------------------------------------------
def scene(B, H, W, depth="smooth", rot=0, tr=0, base=0):
    """(flow fp32 [B,2,H,W], R_true [B,3,3], t_true [B,3], kappa_true [B,H,W]): image b carries rotation (rot + b), translation
    (tr + b) and baseline (base + b) of the lists, over the depth field `depth`; made in float64 and cast."""
    rho = pr.DEPTHS[depth](H, W)
    Rs = [ec.ROTATIONS[(rot + b) % 3][1](W) for b in range(B)]
    ts = [pr.unit(TRANSLATIONS[(tr + b) % 3]) for b in range(B)]
    Ts = [BASELINES[(base + b) % 2] for b in range(B)]
    flow = np.stack([pr.scene_flow(Rs[b], ts[b], Ts[b], rho) for b in range(B)]).astype(np.float32)
    return flow, np.stack(Rs), np.stack(ts), np.stack([T / rho for T in Ts])


def many_scenes(B, H, W):
    """(flow, R_true, t_true) of B images, a different scene each: the 36 combinations of rotation, translation, baseline and depth
    field, and from image 36 on the same again with a quarter of the columns wound one way and a quarter the other (seed b)."""
    out = []
    for b in range(B):
        flow, R, t, _ = scene(1, H, W, ("smooth", "room")[(b // 18) % 2], rot=b, tr=b // 3, base=b // 9)
        out.append((flow if b < 36 else ec.wound(flow, b), R, t))
    return tuple(np.concatenate([o[i] for o in out]) for i in range(3))


def robust_scene(H, W):
    """The issue's robust scene: smooth depth, rotation 0, translation 0, |T| = 0.3, and the block of pr.moved_block moved by a
    further (6, -2) px.  -> (flow fp32 [1,2,H,W], R_true, t_true, block [H,W] bool)"""
    flow, R, t, _ = scene(1, H, W, "smooth", 0, 0, 1)
    f = flow.astype(np.float64)
    blk = pr.moved_block(H, W)
    f[0, 0][blk] += 6.0
    f[0, 1][blk] -= 2.0
    return f.astype(np.float32), R[0], t[0], blk


def polar_scene(H, W, seed):
    """A clean scene with a seeded twentieth of the end points thrown past a pole (v = +-H)."""
    flow, R, t, _ = scene(1, H, W)
    rng = np.random.default_rng(seed)
    hit = rng.random((H, W)) < 0.05
    flow[0, 1][hit] = np.where(rng.random(hit.sum()) < 0.5, -float(H), float(H))
    return flow, R, t


def wound_half(flow, seed):
    """The same flow with u + W on a seeded quarter of the pixels and u - W on another: half of them wound."""
    return ec.wound(flow, seed)


# ---- runners -------------------------------------------------------------------------------------------------------------------
def estimator(lib, B, H, W, device="cpu", **kw):
    from prior_flow_amd.parallax import PoseEstimator
    return PoseEstimator(B, H, W, device, lib=lib, **kw)


def snapshot(est):
    """Everything an estimate leaves behind, as numpy: R, t, stats, the rotation-only R, both sets of sums."""
    return dict(R=est.R.cpu().numpy().copy(), t=est.t.cpu().numpy().copy(), stats=est.stats.cpu().numpy().copy(),
                R0=est.estimator.R.cpu().numpy().copy(), sums=est.sums.cpu().numpy().copy(),
                ego_sums=est.estimator.sums.cpu().numpy().copy())


def estimate(lib, flow, mask=None, init_R=None, init_t=None, device="cpu", est=None, **kw):
    B, _, H, W = flow.shape
    if est is None:
        est = estimator(lib, B, H, W, device, **kw)
    est.estimate(_t(flow, device), _t(mask, device), _t(init_R, device), _t(init_t, device))
    return snapshot(est)


def raw_sums(lib, flow, R, t, mode, mask=None, device="cpu", scale_px=1.0, vote_px=0.25, blocks=0, sums=None):
    """The 22 sums [B,22] of ONE accumulate launch on fresh zeros (or on `sums`)."""
    B = flow.shape[0]
    s = torch.zeros(B, 22, dtype=torch.int64, device=device) if sums is None else sums
    lib.epi_accumulate(_t(flow, device), _t(mask, device), _t(np.asarray(R, np.float32), device),
                       None if t is None else _t(np.asarray(t, np.float32), device), s, mode, scale_px, vote_px, blocks)
    return s.cpu().numpy()


def pmap(lib, flow, R, t, mask=None, device="cpu", **kw):
    """(inv_depth, resid, conf, moving) as numpy, written over NaN / 255 so that a pixel nobody wrote shows."""
    from prior_flow_amd.parallax import parallax_map
    B, _, H, W = flow.shape
    out = tuple(torch.full((B, H, W), float("nan"), device=device) for _ in range(3)) \
        + (torch.full((B, H, W), 255, dtype=torch.uint8, device=device),)
    parallax_map(_t(flow, device), _t(np.asarray(R, np.float32), device), _t(np.asarray(t, np.float32), device), mask=_t(mask, device),
                 out=out, lib=lib, **kw)
    return tuple(o.cpu().numpy() for o in out)


def stepwise(lib, flow, mask=None, init_R=None, init_t=None, device="cpu", t_passes=4, rounds=2, scale_px=1.0, vote_px=0.25,
             gap_min=1e-3, min_parallax_px=0.05, blocks=0, raw=False):
    """The estimate as its entry points called one by one on buffers of the caller: the list of (kind, first, R, t, stats) after
    every pass, preceded by ("rot", False, R0, 0, 0).  raw: also the 22 sums between each accumulate and its solve."""
    from prior_flow_amd.egomotion import RotationEstimator
    from prior_flow_amd import _lib
    B, _, H, W = flow.shape
    f, m, it = _t(flow, device), _t(mask, device), _t(init_t, device)
    rot = RotationEstimator(B, H, W, device, lib=lib, blocks=blocks)
    R = rot.estimate(f, m, _t(init_R, device)).clone()
    t = torch.full((B, 3), float("nan"), device=device)
    stats = torch.full((B, 6), float("nan"), device=device)
    sums = torch.zeros(B, 22, dtype=torch.int64, device=device)
    n = lambda x: x.cpu().numpy().copy()                            # noqa: E731
    out = [("rot", False, n(R), np.zeros((B, 3)), np.zeros((B, 6)))]
    for kind, first in pr.Pose(B, H, W, t_passes=t_passes, rounds=rounds).schedule():
        mode = _lib.EPI_T if kind == "T" else _lib.EPI_R
        lib.epi_accumulate(f, m, R, None if first else t, sums, mode, scale_px, vote_px, blocks)
        mid = n(sums)
        lib.epi_solve(sums, it, R, t, stats, H, W, mode, gap_min, min_parallax_px)
        out.append((kind, first, n(R), n(t), n(stats)) + ((mid,) if raw else ()))
    assert not sums.cpu().numpy().any(), "the solves left sums behind"
    return out


# ---- checks --------------------------------------------------------------------------------------------------------------------
def check_steps(steps, flow, mask=None, init_R=None, init_t=None, what="", fault=None, **kw):
    """Every pass of `steps` (stepwise) against the restatement started from the state the pass before left behind, within the
    single-launch bounds of epipolar_ref; the rotation estimate against egomotion_ref's.  Prints and returns the worst ratio."""
    B, _, H, W = flow.shape
    ref = pr.Pose(B, H, W, fault=fault, **kw)
    R0, st0 = ref.rot.estimate(flow, mask, init_R)
    worst_r0 = 0.0
    for b in range(B):
        bound = er.rotation_bound(st0[b, 3]) if st0[b, 4] else 0.0
        err = er.angle_between(steps[0][2][b], R0[b])
        assert err <= bound, (what, b, "rotation estimate", err, bound)
        worst_r0 = max(worst_r0, err / bound if bound else 0.0)
    worst_t = worst_r = 0.0
    R, t, stats = steps[0][2].astype(np.float64), np.zeros((B, 3)), np.zeros((B, 6))
    for i, (kind, first, gR, gt, gst) in enumerate(s[:5] for s in steps[1:]):
        rR, rt, rst = ref.step(kind, first, flow, mask, R, t, stats, init_t)
        for b in range(B):
            tag = (what, f"pass {i} ({kind})", b)
            if kind == "T":
                assert np.array_equal(gR[b], R[b].astype(np.float32)), tag + ("a T pass touched R",)
                assert gst[b, 5] == rst[b, 5], tag + ("valid", gst[b], rst[b])
                assert gst[b, 2] == np.float32(rst[b, 2]), tag + ("used",)
                if rst[b, 5]:
                    bound = pr.t_pass_bound(rst[b], ref.last_t[b], W, ref.vote_px, ref.scale_px)
                    err = pr.angle_vec(gt[b], rt[b])
                    assert err <= bound, tag + ("t", err, bound)
                    worst_t = max(worst_t, err / bound)
                    assert abs(np.linalg.norm(gt[b].astype(np.float64)) - 1) <= 4 * er.U, tag + ("t is not a unit vector",)
                    # stats: fp32 values of float64 sums whose terms carry NORMAL; the weight's slope is 1.3 / c
                    rel = 1.3 * pr.NORMAL * W / (2 * np.pi * ref.scale_px) + 8 * er.U
                    assert abs(gst[b, 0] - rst[b, 0]) <= rel * rst[b, 0], tag + ("sum w", gst[b, 0], rst[b, 0])
                    assert abs(gst[b, 3] - rst[b, 3]) <= 4 * bound + 8 * er.U, tag + ("gap", gst[b, 3], rst[b, 3])
                    px = W / (2 * np.pi)
                    assert abs(gst[b, 1] - rst[b, 1]) <= 2 * pr.NORMAL * px + rel * rst[b, 1], tag + ("rms e", gst[b, 1], rst[b, 1])
                    assert abs(gst[b, 4] - rst[b, 4]) <= 2 * pr.NORMAL * px + rel * rst[b, 4], tag + ("parallax", gst[b, 4], rst[b, 4])
                else:
                    assert np.array_equal(gt[b], rt[b].astype(np.float32)), tag + ("t of an invalid fit", gt[b], rt[b])
            else:
                assert np.array_equal(gt[b], t[b].astype(np.float32)), tag + ("an R pass touched t",)
                if ref.last_r[b, 1] == 0:
                    assert np.array_equal(gR[b], R[b].astype(np.float32)), tag + ("R moved without a refinement",)
                else:
                    bound = pr.r_pass_bound(ref.last_r[b, 0], ref.last_r[b, 1])
                    err = er.angle_between(gR[b], rR[b])
                    assert err <= bound, tag + ("R", err, bound)
                    worst_r = max(worst_r, err / bound)
                    rt_ = np.abs(gR[b].astype(np.float64).T @ gR[b] - np.eye(3)).max()
                    assert rt_ <= 8 * er.U, tag + ("R is not orthonormal", rt_)
        R, t, stats = gR.astype(np.float64), gt.astype(np.float64), gst.astype(np.float64)    # the chain continues from the code's state
    print(f"[epipolar] {what}: worst error / bound: rotation estimate {worst_r0:.2e}, T passes {worst_t:.2e}, R passes {worst_r:.2e}")
    return max(worst_r0, worst_t, worst_r)


def check_map(got, flow, R, t, ref, what, thr_px=1.0, neg_px=0.5, conf_min=0.05):
    """A parallax map against the restatement's (kappa, resid, conf, moving, a) on the same fp32 R and t.  Returns (worst ratio,
    share of pixels near a threshold)."""
    kappa, resid, conf, moving, a = ref
    gk, gr, gc, gm = got
    W = flow.shape[3]
    for o in (gk, gr, gc):
        assert np.isfinite(o).all(), (what, "not every pixel was written")
    assert set(np.unique(gm)) <= {0, 1}, (what, "moving is not 0 / 1")
    cb = 4 * er.BEARING + 8 * er.U                                  # conf = |q x t|^2 <= 1: q off by BEARING, twice, and the squares
    assert (np.abs(gc - conf) <= cb).all(), (what, "conf", np.abs(gc - conf).max())
    near = np.abs(conf - conf_min) <= cb
    on = (conf >= conf_min) & (conf > 0) & ~near
    off = ~((conf >= conf_min) & (conf > 0)) & ~near
    assert not gk[off].any() and not gr[off].any() and not gm[off].any(), (what, "pixels without an answer are not zero")
    root = np.sqrt(np.where(on, conf, 1.0))
    nn = np.linalg.norm(pr.pixel_terms(flow, R, t, 1.0)["n"], axis=-1)
    kb = 4 * pr.NORMAL * (1 + np.abs(kappa)) / root + 8 * er.U * np.abs(kappa)
    eb = 2 * pr.NORMAL / np.maximum(root - nn, 1e-3)
    rb = eb * W / (2 * np.pi) + 8 * er.U * resid
    ek, erd = np.abs(gk - kappa), np.abs(gr - resid)
    worst = float(max((ek / kb)[on].max(), (erd / rb)[on].max())) if on.any() else 0.0
    assert (ek[on] <= kb[on]).all(), (what, "kappa", worst)
    assert (erd[on] <= rb[on]).all(), (what, "resid", worst)
    near = near | (on & ((np.abs(resid - thr_px) <= rb) | (np.abs(a + neg_px * 2 * np.pi / W) <= 4 * pr.NORMAL / root)))
    diff = gm != moving
    assert not (diff & ~near).any(), (what, "a moving byte differs away from a threshold")
    share = float(near.mean())
    assert share <= MOVING_CAP, (what, "pixels within the bound of a threshold", share)
    print(f"[epipolar] {what}: worst error / bound {worst:.4f}; {int(diff.sum())} moving bytes differ, {share:.2%} of the pixels near a threshold")
    return worst, share
