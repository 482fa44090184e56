"""Seeded inputs and runners shared by tests/test_egomotion_host.py (the host emulation) and tests/test_hip_egomotion.py (the
device): the emulation's handle, one estimate / track / rotate / derotate through the typed wrappers on numpy inputs, and the
checks that hold a result to the float64 restatement (tests/egomotion_ref.py)."""
import ctypes
import functools

import numpy as np
import torch

import egomotion_ref as er
import viewport_ref as vr

SHAPES = ((6, 10), (33, 70), (32, 64), (48, 96))
# (name, R_true(W)): the rotations of the sweep
ROTATIONS = (("axis123_3deg", lambda W: er.axis_angle((1, 2, 3), 3.0)),
             ("axis1m1_120deg", lambda W: er.axis_angle((1, -1, 0.2), 120.0)),
             ("yaw5", lambda W: er.yaw(5, W)))
ENTRIES = ("pf_ego_scratch_bytes", "pf_ego_accumulate", "pf_ego_solve", "pf_ego_track", "pf_erp_rotate", "pf_ego_derotate")


@functools.lru_cache(maxsize=None)
def emu():
    """PfLib handle of tests/emu/libpf_emu_egomotion.so (built on demand): only the six egomotion entry points are present."""
    import __graft_entry__ as ge
    from prior_flow_amd import _lib
    so = ge.build_emu_egomotion()
    lib = _lib.PfLib(so, require_cuda=False, optional=tuple(n for n in _lib.EXPORTS if n not in ENTRIES))
    lib._dll.pf_emu_ego_order.argtypes = [ctypes.c_ulonglong]
    lib._dll.pf_emu_ego_order.restype = None
    lib._dll.pf_emu_ego_scales.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    lib._dll.pf_emu_ego_scales.restype = None
    return lib


def _t(a, device):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def rotation_flows(B, H, W, rot=0):
    """(flow fp32 [B,2,H,W], R_true [B,3,3]): image b carries rotation (rot + b) of ROTATIONS, made in float64 and cast."""
    Rs = [ROTATIONS[(rot + b) % len(ROTATIONS)][1](W) for b in range(B)]
    return np.stack([er.flow_of(R, H, W) for R in Rs]).astype(np.float32), np.stack(Rs)


MANY = 65          # the per-image kernels (solve, track) give a lane to an image: image 64 is the first of a second workgroup


def many_rotation_flows(B, H, W, seed=17):
    """(flow fp32 [B,2,H,W], R [B,3,3]): image b carries rotation b of small_rotations(B, seed), a different one per image."""
    Rs = small_rotations(B, seed).astype(np.float64)
    return np.stack([er.flow_of(R, H, W) for R in Rs]).astype(np.float32), Rs


def grid_flows(B, H, W, seed):
    """(flow fp32 [B,2,H,W], c, r int [B,H,W]): grid inputs.  Every end point is the centre of a pixel (r, c) with c >= x, reached by
    u = c - x (or c - x - W where c > x, on a seeded half) and v = r - y, all whole numbers: x + u mod W and y + v are exact, so
    both bearings of a pixel are built from cosf and sinf of the grid's own H + W angles and from nothing else."""
    rng = np.random.default_rng(seed)
    x, y = np.arange(W)[None, None, :], np.arange(H)[None, :, None]
    c = rng.integers(np.broadcast_to(x, (B, H, W)), W)
    r = rng.integers(0, H, (B, H, W))
    u = (c - x) - np.where((rng.random((B, H, W)) < 0.5) & (c > x), W, 0)
    return np.stack([u, r - y], 1).astype(np.float32), c, r


def grid_agreement(lib, H, W, c, r, device):
    """bool [B,H,W]: the pixels of grid_flows whose own row and column and whose end point's row and column are angles at which
    `lib` on `device` and the host's math library give the same cosf and sinf, bit for bit.  The two sets of values are read off
    pf_seg_tables, which evaluates pf_ego_row and pf_vp_theta's cosf and sinf and nothing else; a clamp of cos phi at 0 that changes
    a value shows as a disagreement.  -> (agree, rows that agree [H], columns that agree [W])"""
    import segments_cases as sc
    (dr, dc), (hr, hc) = sc.tables(lib, H, W, device), sc.tables(sc.emu(), H, W)
    ok_r, ok_c = (sc.bits(dr) == sc.bits(hr)).all(1), (sc.bits(dc) == sc.bits(hc)).all(1)
    return ok_r[None, :, None] & ok_c[None, None, :] & ok_r[r] & ok_c[c], ok_r, ok_c


def wound(flow, seed):
    """The same flow with u + W on a seeded quarter of the pixels and u - W on another."""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 4, flow[:, 0].shape)
    out = flow.astype(np.float64).copy()
    W = flow.shape[3]
    out[:, 0] += np.where(k == 0, W, 0.0) - np.where(k == 1, W, 0.0)
    return out.astype(np.float32)


def robust_flow(H, W):
    """The issue's experiment: 3 degrees about (1, 2, 3); rows H/4..3H/4, columns W/8..W/8 + 0.6 W moved by a further (6, -2) px."""
    R = er.axis_angle((1, 2, 3), 3.0)
    f = er.flow_of(R, H, W)
    x0 = W // 8
    f[0, H // 4:3 * H // 4, x0:x0 + int(0.6 * W)] += 6.0
    f[1, H // 4:3 * H // 4, x0:x0 + int(0.6 * W)] -= 2.0
    return f[None].astype(np.float32), R


def polar_flow(H, W, seed):
    """A rotation flow with a seeded twentieth of the pixels thrown past a pole (v = +-H): the end point clamps to the pole row's
    edge.  For the plain fit (passes = 1), where these pixels count in full."""
    flow, R = rotation_flows(1, H, W)
    rng = np.random.default_rng(seed)
    hit = rng.random((H, W)) < 0.05
    flow[0, 1][hit] = np.where(rng.random(hit.sum()) < 0.5, -float(H), float(H))
    return flow, R


def poison(flow, seed):
    """(flow with NaN, +-inf and 1e30 on a seeded tenth of the pixels, the mask of those pixels)."""
    rng = np.random.default_rng(seed)
    bad = rng.random(flow[:, 0].shape) < 0.1
    junk = rng.choice(np.array([np.nan, np.inf, -np.inf, 1e30, -1e30], np.float32), size=flow.shape)
    ch = rng.integers(0, 3, flow[:, 0].shape)                   # u, v or both
    out = flow.copy()
    out[:, 0] = np.where(bad & (ch != 1), junk[:, 0], out[:, 0])
    out[:, 1] = np.where(bad & (ch != 0), junk[:, 1], out[:, 1])
    return out, bad.astype(np.uint8)


def smooth_frame(B, C, H, W, seed, byte=False):
    """A smooth seeded frame [B,C,H,W]: a few low harmonics of the sphere, 0..255; as fp32, or as bytes [B,H,W,C]."""
    rng = np.random.default_rng(seed)
    m, n = er.grid(H, W)
    s = vr.sphere(m, n, H, W)
    out = np.zeros((B, C, H, W))
    for b in range(B):
        for c in range(C):
            k = rng.normal(size=(3,))
            k2 = rng.normal(size=(3,))
            out[b, c] = 127.5 + 60 * (s @ (k / np.linalg.norm(k))) + 40 * (s @ (k2 / np.linalg.norm(k2))) ** 2
    if byte:
        return np.ascontiguousarray(np.clip(np.floor(out + 0.5), 0, 255).astype(np.uint8).transpose(0, 2, 3, 1))
    return out.astype(np.float32)


def small_rotations(n, seed):
    """n seeded rotations as fp32 matrices: up to 4 degrees about a random axis on top of a drift of 1 degree about (2, 1, 3), so
    that the orientation turns through several full circles and the scalar part of its quaternion changes sign."""
    rng = np.random.default_rng(seed)
    drift = er.axis_angle((2, 1, 3), 1.0)
    return np.stack([(er.axis_angle(rng.normal(size=3), rng.uniform(0, 4)) @ drift) for _ in range(n)]).astype(np.float32)


# ---- runners -------------------------------------------------------------------------------------------------------------------
def estimate(lib, flow, mask=None, init=None, device="cpu", passes=4, scale_px=1.0, gap_min=1e-3, blocks=0, est=None):
    """(R [B,3,3], stats [B,5], sums afterwards [B,12]) as numpy through RotationEstimator; est: an estimator to reuse."""
    from prior_flow_amd.egomotion import RotationEstimator
    B, _, H, W = flow.shape
    if est is None:
        est = RotationEstimator(B, H, W, device, passes=passes, scale_px=scale_px, gap_min=gap_min, lib=lib, blocks=blocks)
    R = est.estimate(_t(flow, device), _t(mask, device), _t(init, device))
    return R.cpu().numpy().copy(), est.stats.cpu().numpy().copy(), est.sums.cpu().numpy().copy()


def raw_sums(lib, flow, R, weighted, mask=None, device="cpu", scale_px=1.0, blocks=0):
    """The twelve sums [B,12] of ONE accumulate launch on fresh zeros."""
    B = flow.shape[0]
    sums = torch.zeros(B, 12, dtype=torch.int64, device=device)
    lib.ego_accumulate(_t(flow, device), _t(mask, device), _t(np.asarray(R, np.float32), device), sums, weighted, scale_px, blocks)
    return sums.cpu().numpy()


def track(lib, Rs, smoothing, device="cpu"):
    """The tracker over a sequence Rs [T,3,3] of one video: (orientations [T,3,3], corrections [T,3,3], states [T,8]); over
    Rs [T,B,3,3] of B videos in one batch: the same with [T,B,...]."""
    Rs = np.asarray(Rs, np.float32)
    one = Rs.ndim == 3
    seq = _t(Rs[:, None] if one else Rs, device)
    B = seq.shape[1]
    state = torch.zeros(B, 8, dtype=torch.float64, device=device)
    state[:, 0::4] = 1.0
    o = torch.zeros(B, 3, 3, device=device)
    c = torch.zeros(B, 3, 3, device=device)
    O, Cc, S = [], [], []
    for t in range(seq.shape[0]):
        lib.ego_track(seq[t], state, o, c, smoothing)
        O.append(o.clone()), Cc.append(c.clone()), S.append(state.clone())
    return tuple((torch.cat(x) if one else torch.stack(x)).cpu().numpy() for x in (O, Cc, S))


def rotate(lib, frame, R, device="cpu"):
    from prior_flow_amd.egomotion import rotate_erp
    fill = float("nan") if frame.dtype == np.float32 else 255
    out = torch.full(frame.shape, fill, dtype=torch.from_numpy(frame[:1]).dtype, device=device)
    return rotate_erp(_t(frame, device), _t(np.asarray(R, np.float32), device), out=out, lib=lib).cpu().numpy()


def derotate(lib, flow, R, mask=None, device="cpu"):
    from prior_flow_amd.egomotion import derotate_flow
    B, _, H, W = flow.shape
    valid = torch.full((B, H, W), 255, dtype=torch.uint8, device=device)
    out = torch.full(flow.shape, float("nan"), dtype=torch.float32, device=device)
    derotate_flow(_t(flow, device), _t(np.asarray(R, np.float32), device), valid=valid, mask=_t(mask, device), out=out, lib=lib)
    return out.cpu().numpy(), valid.cpu().numpy()


# ---- checks --------------------------------------------------------------------------------------------------------------------
def check_rotation(got_R, got_stats, ref, what):
    """R and stats of every image against the float64 statement's (R, stats); prints and returns the worst angle / bound."""
    ref_R, ref_stats = ref
    worst = 0.0
    for b in range(len(ref_R)):
        assert got_stats[b, 4] == ref_stats[b, 4], (what, b, "valid", got_stats[b], ref_stats[b])
        bound = er.rotation_bound(ref_stats[b, 3]) if ref_stats[b, 4] else 0.0
        err = er.angle_between(got_R[b], ref_R[b])
        worst = max(worst, err / bound if bound else float(err > 0))
        assert err <= bound, (what, b, "angle", err, bound)
        rt = np.abs(got_R[b].astype(np.float64).T @ got_R[b] - np.eye(3)).max()
        assert rt <= 8 * er.U, (what, b, "R is not orthonormal", rt)
        # sum w, rms chord, used fraction, gap: fp32 values of float64 sums whose terms carry the bearings' rounding
        assert abs(got_stats[b, 0] - ref_stats[b, 0]) <= 4 * er.BEARING * ref_stats[b, 0] + 1e-30, (what, b, "sum w")
        assert abs(got_stats[b, 1] - ref_stats[b, 1]) <= 4 * er.BEARING + 4 * er.U * ref_stats[b, 1], (what, b, "rms", got_stats[b, 1], ref_stats[b, 1])
        assert got_stats[b, 2] == np.float32(ref_stats[b, 2]), (what, b, "used")
        assert abs(got_stats[b, 3] - ref_stats[b, 3]) <= 64 * er.BEARING, (what, b, "gap", got_stats[b, 3], ref_stats[b, 3])
    print(f"[egomotion] {what}: worst angle / bound {worst:.4f}")
    return worst


def check_derotated(got, got_valid, flow, R, ref, what):
    """A derotated flow against the statement's (flow', valid): valid equal, exactly (0, 0) where left out, the end points on
    the sphere within the chord bound, u' inside [-W/2, W/2), and in pixels where the sphere is not degenerate (|phi| < 60 deg)."""
    want, wvalid = ref
    B, _, H, W = flow.shape
    assert np.array_equal(got_valid, wvalid), (what, "valid")
    off = wvalid == 0
    assert not got[:, 0][off].any() and not got[:, 1][off].any(), (what, "left-out pixels are not (0, 0)")
    m, n = er.grid(H, W)
    a = vr.sphere(m + got[:, 0].astype(np.float64), n + got[:, 1].astype(np.float64), H, W)
    b = vr.sphere(m + want[:, 0], n + want[:, 1], H, W)
    chord = np.where(off, 0.0, np.linalg.norm(a - b, axis=-1))
    worst = float(chord.max() / er.CHORD)
    assert worst <= 1.0, (what, "chord", chord.max(), er.CHORD)
    assert (got[:, 0] >= -W / 2).all() and (got[:, 0] <= W / 2).all(), (what, "u' outside [-W/2, W/2]")
    phi = (0.5 - (n + 0.5) / H) * np.pi
    low = (np.abs(phi) < np.pi / 3)[None] & ~off
    du = np.abs(got[:, 0] - want[:, 0])
    px = er.CHORD * W / (2 * np.pi * 0.5)
    near_seam = np.abs(np.abs(want[:, 0]) - W / 2) <= px            # a u' this near to +-W/2 may wrap the other way
    assert (du[low & ~near_seam] <= px).all(), (what, "u' in pixels", du[low & ~near_seam].max(), px)
    print(f"[egomotion] {what}: worst chord / bound {worst:.4f}")
    return worst


def check_rotated(got, frame, R, ref, what):
    """An fp32 frame resampled under R against the statement under the value bound; prints and returns the worst ratio."""
    bound = er.value_bound(frame, R)
    err = np.abs(got.astype(np.float64) - ref)
    assert np.isfinite(got).all(), (what, "not every pixel was written")
    worst = float((err / bound).max())
    assert worst <= 1.0, (what, float(err.max()), worst)
    print(f"[egomotion] {what}: worst error / bound {worst:.4f}")
    return worst


def check_rotated_u8(got, frame, R, ref, what):
    """The byte form: at most 1 count of difference, only where the float64 value lies within the bound of a half, and at most
    2 % of the bytes differ at all."""
    val, want = ref
    bound = er.value_bound(frame.astype(np.float64).transpose(0, 3, 1, 2), R).transpose(0, 2, 3, 1)
    diff = np.abs(got.astype(np.int64) - want.astype(np.int64))
    near = np.abs(val + 0.5 - np.round(val + 0.5)) <= bound
    assert diff.max() <= 1, (what, int(diff.max()))
    assert not (diff[~near] != 0).any(), (what, "a byte differs away from a half")
    share = float((diff != 0).mean())
    assert share <= 0.02, (what, share)
    print(f"[egomotion] {what}: {share:.2%} of the bytes differ by one count; {float(near.mean()):.2%} lie within the bound of a half")
    return share
