"""Seeded scenes and runners shared by tests/test_odometry_host.py (the host emulation) and tests/test_hip_odometry.py (the device):
the emulation's handle, links / tracks / fusions through the typed wrappers on numpy inputs, and the checks that hold a result to
the float64 restatement (tests/odometry_ref.py).

The scenes come from epipolar_ref's generators.  Two consecutive pairs k and k + 1 share a frame with depth rho: the backward flow
of pair k is scene_flow(R_k^T, -R_k^T t_k, T_k, rho), the forward flow of pair k + 1 is scene_flow(R_k+1, t_k+1, T_k+1, rho), both on
the shared frame's grid.  The forward flow of pair k, which only the pose estimate reads, is scene_flow(R_k, t_k, T_k, rho') over
the depth rho' of the frame before.  The two flows of ONE pair are never compared pixel by pixel here, so they need not show one
surface (and with two different depth fields they do not)."""
import ctypes
import functools

import numpy as np
import torch

import egomotion_cases as ec
import egomotion_ref as er
import epipolar_cases as pc
import epipolar_ref as pr
import odometry_ref as orf

SHAPES = ec.SHAPES
BASELINES = (0.1, 0.2, 0.3)
ENTRIES = pc.ENTRIES + ("pf_odo_hist_bytes", "pf_odo_accumulate", "pf_odo_solve", "pf_odo_reverse_pose", "pf_odo_track", "pf_odo_fuse")
NEAR_CAP = pc.MOVING_CAP           # the share of pixels that may lie within the rounding of a bin edge
_t = ec._t


@functools.lru_cache(maxsize=None)
def emu():
    """PfLib handle of tests/emu/libpf_emu_odometry.so (built on demand): the odometry entry points and the pose entry points a
    whole Odometry needs."""
    import __graft_entry__ as ge
    from prior_flow_amd import _lib
    so = ge.build_emu_odometry()
    lib = _lib.PfLib(so, require_cuda=False, optional=tuple(n for n in _lib.EXPORTS if n not in ENTRIES))
    lib._dll.pf_emu_odo_order.argtypes = [ctypes.c_ulonglong]
    lib._dll.pf_emu_odo_order.restype = None
    lib._dll.pf_emu_odo_worst.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_longlong)]
    lib._dll.pf_emu_odo_worst.restype = None
    lib._dll.pf_emu_odo_rows.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_float)]
    lib._dll.pf_emu_odo_rows.restype = None
    return lib


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else (a.view(np.uint64) if a.dtype == np.float64 else a)


# ---- scenes ----------------------------------------------------------------------------------------------------------------------
def motion(W, rot, tr, T):
    """(R, t, T) number (rot, tr) of the sweeps of epipolar_cases with baseline T."""
    return ec.ROTATIONS[rot % 3][1](W), pr.unit(pc.TRANSLATIONS[tr % 3]), float(T)


def pair_flows(H, W, mk, mk1, depth="smooth", depth_before="room"):
    """fp32 [2,H,W] each: (forward flow of pair k over depth_before, backward flow of pair k and forward flow of pair k + 1 over
    `depth`, the depth of the frame the two pairs share)."""
    rho, rho0 = pr.DEPTHS[depth](H, W), pr.DEPTHS[depth_before](H, W)
    (R0, t0, T0), (R1, t1, T1) = mk, mk1
    fwd0 = pr.scene_flow(R0, t0, T0, rho0)
    bwd0 = pr.scene_flow(R0.T, -R0.T @ t0, T0, rho)
    fwd1 = pr.scene_flow(R1, t1, T1, rho)
    return tuple(f.astype(np.float32) for f in (fwd0, bwd0, fwd1))


def move_block(flow, blk, dx=6.0, dy=-2.0, shift=0):
    """The flow [2,H,W] with the block (shifted by `shift` columns) moved by a further (dx, dy) px."""
    f = flow.astype(np.float64)
    b = np.roll(blk, shift, axis=1)
    f[0][b] += dx
    f[1][b] += dy
    return f.astype(np.float32), b


def true_maps(bwd0, fwd1, mk, mk1, mapper):
    """Maps a and b (kappa, conf, moving) [1,H,W] under the TRUE poses through `mapper(flow [1,2,H,W], R [1,3,3], t [1,3])`."""
    (R0, t0, _), (R1, t1, _) = mk, mk1
    return mapper(bwd0[None], R0.T[None], (-R0.T @ t0)[None]), mapper(fwd1[None], R1[None], t1[None])


def many_maps(B, H, W, mapper):
    """Maps a and b [B,H,W] of B images under the true poses, a different scene per image: the nine pairs of motions, the four
    ordered pairs of baselines whose ratio is no power of two (such a ratio puts l ON a bin edge) and the two depth fields, 72
    combinations."""
    pairs = ((0.1, 0.3), (0.3, 0.2), (0.2, 0.3), (0.3, 0.1))
    assert B <= 72
    maps = []
    for b in range(B):
        Ta, Tb = pairs[(b // 9) % 4]
        mk, mk1 = motion(W, b, b // 3 + 1, Ta), motion(W, b + 1, b // 3, Tb)
        _, bwd0, fwd1 = pair_flows(H, W, mk, mk1, ("smooth", "room")[(b // 36) % 2])
        maps.append(true_maps(bwd0, fwd1, mk, mk1, mapper))
    return tuple(tuple(np.concatenate([m[s][i] for m in maps]) for i in range(3)) for s in (0, 1))


def ref_mapper(flow, R, t, mask=None):
    k, _, c, m, _ = pr.parallax(flow, np.asarray(R, np.float32), np.asarray(t, np.float32), mask)
    return k.astype(np.float32), c.astype(np.float32), m


def lib_mapper(lib, device="cpu"):
    def run(flow, R, t, mask=None):
        k, _, c, m = pc.pmap(lib, flow, R, t, mask, device)
        return k, c, m
    return run


def grid_maps(B, H, W, bins, L, seed, integer=False):
    """Grid inputs: kappa_a a power of two, kappa_b = kappa_a 2^l with l at bin centres (integer: at whole numbers, which log2f
    returns exactly), conf in (0, 1.5], a tenth of the pixels moving in one map or the other.  -> (map_a, map_b, l [B,H,W])"""
    rng = np.random.default_rng(seed)
    ka = np.exp2(rng.integers(-6, 4, (B, H, W))).astype(np.float32)
    if integer:
        l = rng.integers(-3, 4, (B, H, W)).astype(np.float64)
    else:
        l = (rng.integers(1, bins - 1, (B, H, W)) + 0.5) * (2 * L / bins) - L
    kb = (ka.astype(np.float64) * np.exp2(l)).astype(np.float32)
    ca, cb = (rng.integers(1, 97, (B, H, W)) / 64).astype(np.float32), (rng.integers(1, 97, (B, H, W)) / 64).astype(np.float32)
    mv = rng.random((B, H, W))
    return (ka, ca, (mv < 0.05).astype(np.uint8)), (kb, cb, (mv > 0.95).astype(np.uint8)), l


# ---- runners -------------------------------------------------------------------------------------------------------------------
def dev_map(m, device):
    return tuple(_t(np.ascontiguousarray(x), device) for x in m)


def link_run(lib, map_a, map_b, device="cpu", blocks=0, hist=None, **opt):
    """One accumulate and one solve on fresh zeros (or on `hist`): (ratio [B], stats [B,6], cells before the solve, after it)."""
    o = dict(orf.DEFAULTS, **opt)
    B, H, W = map_a[0].shape
    h = torch.zeros(B, 2 * o["bins"] + 2, dtype=torch.int64, device=device) if hist is None else hist
    ratio = torch.full((B,), float("nan"), device=device)
    stats = torch.full((B, 6), float("nan"), device=device)
    lib.odo_accumulate(dev_map(map_a, device), dev_map(map_b, device), h, o["bins"], o["log2_range"], o["kappa_min"], blocks)
    mid = h.cpu().numpy().copy()
    lib.odo_solve(h, ratio, stats, H, W, o["bins"], o["log2_range"], o["trim_bins"], o["min_used"], o["max_iqr"])
    return ratio.cpu().numpy(), stats.cpu().numpy(), mid, h.cpu().numpy()


def reverse_run(lib, R, t, device="cpu"):
    R, t = _t(np.asarray(R, np.float32), device), _t(np.asarray(t, np.float32), device)
    Rr, tr = torch.full_like(R, float("nan")), torch.full_like(t, float("nan"))
    lib.odo_reverse_pose(R, t, Rr, tr)
    return Rr.cpu().numpy(), tr.cpu().numpy()


class TrackRun:
    """pf_odo_track on buffers of its own, fed with numpy."""

    def __init__(self, lib, B, device="cpu"):
        from prior_flow_amd.odometry import _STATE0
        self.lib, self.B, self.device = lib, B, device
        self.state = torch.tensor(_STATE0, dtype=torch.float64, device=device).repeat(B, 1).contiguous()
        self.out = (torch.full((B, 3, 3), float("nan"), device=device), torch.full((B, 3), float("nan"), device=device),
                    torch.full((B,), float("nan"), device=device), torch.full((B, 4), -1, dtype=torch.int32, device=device))

    def step(self, R, t, pose_valid, ratio, link_valid):
        d, B = self.device, self.B
        ps, ls = np.zeros((B, 6), np.float32), np.zeros((B, 6), np.float32)
        ps[:, 5], ls[:, 5] = pose_valid, link_valid
        self.lib.odo_track(_t(np.asarray(R, np.float32), d), _t(np.asarray(t, np.float32), d), _t(ps, d), _t(np.asarray(ratio, np.float32), d),
                           _t(ls, d), self.state, *self.out)
        return tuple(o.cpu().numpy().copy() for o in self.out)


def fuse_run(lib, map_a, map_b, S_a, S_b, link_valid, device="cpu", **kw):
    from prior_flow_amd.odometry import fuse_depth
    B, H, W = map_a[0].shape
    out = (torch.full((B, H, W), float("nan"), device=device), torch.full((B, H, W), float("nan"), device=device),
           torch.full((B, H, W), 255, dtype=torch.uint8, device=device))
    fuse_depth(dev_map(map_a, device), dev_map(map_b, device), _t(np.asarray(S_a, np.float32), device), _t(np.asarray(S_b, np.float32), device),
               _t(np.asarray(link_valid, np.float32), device), out=out, lib=lib, **kw)
    return tuple(o.cpu().numpy() for o in out)


# ---- checks --------------------------------------------------------------------------------------------------------------------
def _flip(cells, k, n, shift):
    """Whether moving a weight `shift` across bin edges can change the first bin with k C >= n total."""
    C = np.cumsum(cells)
    tot = C[-1]
    i = int(np.argmax(k * C >= n * tot))
    above = k * C[i] - n * tot
    below = n * tot - k * C[i - 1] if i > 0 else np.inf
    return min(above, below) <= (k + n) * shift


def check_link(got, map_a, map_b, what, cap=NEAR_CAP, **opt):
    """(ratio, stats, cells before the solve, cells after it) of link_run against the restatement on the same fp32 maps.  Returns
    (worst error / bound, share of pixels near a bin edge).  cap: the largest such share (None: only printed -- a scene whose true
    ratio is a power of two, equal baselines included, has its l ON a bin edge, and its pixels fall to either side)."""
    o = dict(orf.DEFAULTS, **opt)
    bins, L, trim = o["bins"], o["log2_range"], o["trim_bins"]
    ratio, stats, mid, after = got
    B, H, W = map_a[0].shape
    assert not after.any(), (what, "the solve left cells behind")
    rr, rs, d = orf.link(map_a, map_b, **o)
    k = d["terms"]
    inv = er_scale_inv(H, W)
    worst, share = 0.0, float(k["near"].sum() / max(k["used"].sum(), 1))
    assert cap is None or share <= cap, (what, "pixels within the rounding of a bin edge", share)
    for b in range(B):
        Wc, Mc = mid[b, :bins], mid[b, bins:2 * bins]
        assert int(Wc.sum()) == int(mid[b, 2 * bins]), (what, b, "sum of the bins is not the total")
        assert int(mid[b, 2 * bins + 1]) == int(d["count"][b]), (what, b, "count", mid[b, 2 * bins + 1], d["count"][b])
        cnt = np.bincount(k["bin"][b][k["used"][b]], minlength=bins).astype(np.float64)
        nearw = np.bincount(k["bin"][b][k["near"][b]], weights=k["w"][b][k["near"][b]], minlength=bins)
        three = lambda v: v + np.r_[0.0, v[:-1]] + np.r_[v[1:], 0.0]            # noqa: E731
        slack = three(nearw) * (1 + orf.W_REL) + three(cnt) * (orf.W_ABS + inv) + three(d["W"][b]) * orf.W_REL
        ew = np.abs(Wc * inv - d["W"][b])
        em = np.abs(Mc * inv - d["M"][b])
        mslack = slack + three(d["W"][b]) * (orf.edge_rounding(L) / L + 2 * orf.U)
        assert (ew <= slack).all() and (em <= mslack).all(), (what, b, "a bin differs by more than its edge pixels", (ew - slack).max(), (em - mslack).max())
        tb = orf.W_ABS * d["count"][b] + orf.W_REL * d["total"][b] + inv * d["count"][b]
        assert abs(float(stats[b, 0]) - d["total"][b]) <= tb + 2 * orf.U * d["total"][b], (what, b, "sum w")
        assert stats[b, 1] == np.float32(d["count"][b] / (H * W)), (what, b, "used")
        if d["total"][b] == 0:
            assert ratio[b] == 1 and stats[b, 5] == 0 and not stats[b, 2:5].any(), (what, b, "nothing counted")
            continue
        shift = nearw.sum() + tb
        flips = [_flip(d["W"][b], kk, n, shift) for kk, n in ((2, 1), (4, 1), (4, 3))]
        inf = d["info"][b]
        binw = 2 * L / bins
        assert abs(stats[b, 3] - rs[b, 3]) <= (flips[1] + flips[2]) * binw + 4 * orf.U * rs[b, 3], (what, b, "iqr", stats[b, 3], rs[b, 3])
        bound, _ = orf.lhat_bound(d, b, bins, L, trim)
        if flips[0]:
            bound += (2 * trim + 1) * binw
        err = abs(float(stats[b, 2]) - rs[b, 2])
        assert err <= bound + 2 * orf.U * abs(rs[b, 2]), (what, b, "l^", err, bound, inf)
        worst = max(worst, err / bound)
        if not any(flips) and rs[b, 5] == stats[b, 5] == 1:
            rb = np.exp2(bound) - 1 + 2 * orf.U
            assert abs(ratio[b] / rr[b] - 1) <= rb, (what, b, "ratio", ratio[b], rr[b])
        if not any(flips):
            assert stats[b, 5] == rs[b, 5] or abs(rs[b, 1] - o["min_used"]) < 1e-6, (what, b, "valid", stats[b], rs[b])
    print(f"[odometry] {what}: worst error / bound of l^ {worst:.2e}; {share:.2%} of the used pixels near a bin edge")
    return worst, share


def er_scale_inv(H, W):
    """2^-S of pf_ego_scales(H, W)."""
    lg = 0
    while (1 << lg) < H * W:
        lg += 1
    return 2.0 ** -(62 - lg)


def check_fuse(got, map_a, map_b, S_a, S_b, lv, what, **kw):
    inv, ws, dis = got
    rinv, rws, rdis, near, scale = orf.fuse(map_a, map_b, np.asarray(S_a, np.float32), np.asarray(S_b, np.float32), lv, **kw)
    assert np.isfinite(inv).all() and np.isfinite(ws).all() and set(np.unique(dis)) <= {0, 1}, (what, "not every element was written")
    e = np.abs(inv - rinv)
    b = 6 * orf.U * scale
    assert (e <= b).all(), (what, "inv_depth", float((e - b).max()))
    assert (np.abs(ws - rws) <= 2 * orf.U * rws).all(), (what, "weight")
    assert not ((dis != rdis) & ~near).any(), (what, "a disagree byte differs away from the threshold")
    worst = float((e[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0
    print(f"[odometry] {what}: fuse worst error / bound {worst:.3f}; {int((dis != rdis).sum())} disagree bytes differ, {near.mean():.2%} near the threshold")
    return worst


# ---- paths ---------------------------------------------------------------------------------------------------------------------
def path_motions(W, baselines=(0.3, 0.1, 0.2, 0.3), still=None):
    """One motion per pair; `still`: the index of a pair that only rotates (T = 0)."""
    return [motion(W, k, k + 1, 0.0 if k == still else T) for k, T in enumerate(baselines)]


def path_flows(H, W, motions):
    """[(forward, backward)] fp32 [1,2,H,W] per pair: frame j has depth smooth (j even) or room (j odd); the forward flow of pair k
    lies on frame k, its backward flow on frame k + 1."""
    out = []
    for k, (R, t, T) in enumerate(motions):
        rho_k, rho_k1 = (pr.DEPTHS["smooth" if j % 2 == 0 else "room"](H, W) for j in (k, k + 1))
        out.append((pr.scene_flow(R, t, T, rho_k).astype(np.float32)[None], pr.scene_flow(R.T, -R.T @ t, T, rho_k1).astype(np.float32)[None]))
    return out


def path_truth(motions):
    """[(orientation, centre in units of the first baseline of the segment, baseline in those units)] after every pair."""
    A, b, out, unit = np.eye(3), np.zeros(3), [], None
    for R, t, T in motions:
        A, b = R @ A, R @ b + T * t
        if unit is None and T > 0:
            unit = T
        out.append((A.copy(), -A.T @ b / (unit or 1.0), T / (unit or 1.0)))
    return out


def run_path(lib, flows, device="cpu", **kw):
    """Odometry.push_flows over the pairs: [dict(orientation, centre, baseline, flags, ratio, link_stats, inv_depth, weight, disagree)]"""
    from prior_flow_amd.odometry import Odometry
    _, _, H, W = flows[0][0].shape
    odo = kw.pop("odo", None) or Odometry(1, H, W, device, lib=lib, **kw)
    out = []
    for fwd, bwd in flows:
        odo.push_flows(_t(fwd, device), _t(bwd, device))
        out.append({k: getattr(odo, k).cpu().numpy().copy() for k in ("orientation", "centre", "baseline", "flags", "ratio", "link_stats",
                                                                       "inv_depth", "depth_weight", "disagree")})
        out[-1]["pose"] = (odo.pose.R.cpu().numpy().copy(), odo.pose.t.cpu().numpy().copy(), odo.pose.stats.cpu().numpy().copy())
    return out


def ref_path(flows, fault=None):
    """The same chain on the float64 restatement: pr.Pose, pr.parallax, orf.link, orf.Track."""
    _, _, H, W = flows[0][0].shape
    pose, trk, map_a, out = pr.Pose(1, H, W), orf.Track(1, fault), None, []
    for fwd, bwd in flows:
        R, t, st, _ = pose.estimate(fwd)
        kb, _, cb, mb, _ = pr.parallax(fwd, R, t)
        if map_a is None:
            ratio, lst = np.ones(1), np.zeros((1, 6))
        else:
            ratio, lst, _ = orf.link(map_a, (kb, cb, mb), fault=fault)
        A, c, S, fl = trk.step(R, t, st[:, 5], ratio, lst[:, 5])
        Rr, tr = orf.reverse_pose(R, t)
        ka, _, ca, ma, _ = pr.parallax(bwd, Rr, tr)
        map_a = (ka, ca, ma)
        out.append(dict(orientation=A, centre=c, baseline=S, flags=fl, ratio=ratio, link_stats=lst, pose=(R, t, st)))
    return out


# ---- fused depth against the truth -----------------------------------------------------------------------------------------------
def fused_scene(lib, H, W, device="cpu", move=False):
    """Two pairs over the smooth depth, |T| 0.3 then 0.1, every step through `lib` with ESTIMATED poses: dict(ma, mb: the maps of
    the shared frame; pose_a: the reversed pose of the first pair, pose_b: the pose of the second; ratio, stats: the link; S_a,
    S_b, lv; fused: (inv_depth, weight, disagree); mk, mk1, kap = |T_first| / rho, flows).  move: the block moved in the second
    pair only."""
    mk, mk1 = motion(W, 0, 0, 0.3), motion(W, 1, 1, 0.1)
    fwd0, bwd0, fwd1 = pair_flows(H, W, mk, mk1, "smooth")
    if move:
        fwd1, _ = move_block(fwd1, pr.moved_block(H, W))
    e0, e1 = pc.estimate(lib, fwd0[None], device=device), pc.estimate(lib, fwd1[None], device=device)
    Rr, tr = reverse_run(lib, e0["R"], e0["t"], device)
    mapper = lib_mapper(lib, device)
    ma, mb = mapper(bwd0[None], Rr, tr), mapper(fwd1[None], e1["R"], e1["t"])
    ratio, stats, _, _ = link_run(lib, ma, mb, device)
    S_a, S_b, lv = np.ones(1, np.float32), ratio.astype(np.float32), stats[:, 5]
    return dict(ma=ma, mb=mb, pose_a=(Rr, tr), pose_b=(e1["R"], e1["t"]), ratio=ratio, stats=stats, S_a=S_a, S_b=S_b, lv=lv,
                fused=fuse_run(lib, ma, mb, S_a, S_b, lv, device), mk=mk, mk1=mk1, kap=0.3 / pr.DEPTHS["smooth"](H, W),
                flows=(fwd0, bwd0, fwd1))


def fused_tolerance(s, W, conf_min=0.05):
    """(tolerance [H,W] of |inv_depth - |T_first| / rho| in units of the first baseline, counted [H,W] bool): section 20's kappa
    sensitivity 4 (dt + dR + 4 NORMAL)(1 + kappa) / sqrt(max(conf, 0.05)) of EACH map with the pose errors MEASURED on this run
    (map a: the reversed pose of the first pair against (R_0^T, -R_0^T t_0); map b: the second pair's against (R_1, t_1)), map b's
    brought to the first baseline by its S and widened by the measured link error times kappa.  The fused value is a convex
    combination, so where both maps count the larger of the two holds, elsewhere the one that counts."""
    (R0, t0, T0), (R1, t1, T1) = s["mk"], s["mk1"]
    kap = s["kap"]
    link_err = abs(float(s["ratio"][0]) / (T1 / T0) - 1)
    tols = []
    for (R, t), (Rt, tt), m, kt, S in ((s["pose_a"], (R0.T, -R0.T @ t0), s["ma"], kap, 1.0),
                                       (s["pose_b"], (R1, t1), s["mb"], kap * T1 / T0, float(s["S_b"][0]))):
        turn = pr.angle_vec(t[0], tt) + er.angle_between(R[0], Rt) + 4 * pr.NORMAL
        tols.append(4 * turn * (1 + kt) / np.sqrt(np.maximum(m[1][0], conf_min)) / S)
    tols[1] = tols[1] + link_err * kap
    ca = (s["ma"][2][0] == 0) & (s["ma"][1][0] >= np.float32(conf_min)) & (s["lv"][0] != 0)
    cb = (s["mb"][2][0] == 0) & (s["mb"][1][0] >= np.float32(conf_min))
    tol = np.where(ca & cb, np.maximum(tols[0], tols[1]), np.where(ca, tols[0], tols[1]))
    return tol, ca | cb, link_err


def fused_worst(inv, s, W):
    """The worst |inv_depth - kappa| / tolerance over the counted pixels of fused_scene's dict."""
    tol, on, _ = fused_tolerance(s, W)
    return float((np.abs(np.asarray(inv, np.float64)[0] - s["kap"]) / tol)[on].max())


# ---- grid inputs as integers -------------------------------------------------------------------------------------------------------
def scale_of(H, W):
    return 1.0 / er_scale_inv(H, W)


def rows_of(lib, H, W, device="cpu"):
    """cos phi of every row as `lib` computes it (fp32 [H]), read off pf_odo_accumulate itself: image y of a batch of H has ONE used
    pixel, in row y, with conf 1 and equal kappa, so its total cell is quant(cos phi(y)) = cos phi(y) 2^S exactly (an fp32 value
    times a power of two that makes it a whole number)."""
    one = np.ones((H, H, W), np.float32)
    mv = np.ones((H, H, W), np.uint8)
    mv[np.arange(H), np.arange(H), 0] = 0
    h = torch.zeros(H, 2 * 64 + 2, dtype=torch.int64, device=device)
    lib.odo_accumulate(dev_map((one, one, mv), device), dev_map((one, one, mv), device), h, 64, 4.0, 1e-4, 0)
    h = h.cpu().numpy()
    assert (h[:, 129] == 1).all() and (h[:, 32] == h[:, 128]).all()
    rows = (h[:, 128].astype(np.float64) / scale_of(H, W)).astype(np.float32)
    assert (rows.astype(np.float64) * scale_of(H, W) == h[:, 128]).all()
    return rows


def grid_integers(ma, mb, l, rows, bins, L, integer):
    """The cells [B, 2 bins + 2] of grid inputs as the statement's integers, from fp32 arithmetic spelled out in numpy with the
    library's own rows (the weight is a product of an fp32 cosine and two conf values of seven bits, rounded twice as the
    statement does; the bin is exact because l is half a bin from every edge, or whole); M only with whole l, where log2f is exact
    (elsewhere zeros).  -> (cells, used [B,H,W])"""
    B, H, W = ma[0].shape
    scale = scale_of(H, W)
    k = orf.link_terms(ma, mb, bins, L, rows=rows)
    assert integer or not k["near"].any()                               # a whole l lies ON an edge, but every step to its bin is exact
    one = np.float32(1)
    w32 = ((rows[None, :, None] * np.minimum(ma[1], one)).astype(np.float32) * np.minimum(mb[1], one)).astype(np.float32)
    qw = np.rint(w32.astype(np.float64) * scale).astype(np.int64)
    qm = np.rint(((w32 * l.astype(np.float32)).astype(np.float32) / np.float32(L)).astype(np.float64) * scale).astype(np.int64)
    cells = np.zeros((B, 2 * bins + 2), np.int64)
    for b in range(B):
        u = k["used"][b]
        np.add.at(cells[b], k["bin"][b][u], qw[b][u])
        if integer:
            np.add.at(cells[b], bins + k["bin"][b][u], qm[b][u])
        cells[b, 2 * bins], cells[b, 2 * bins + 1] = qw[b][u].sum(), u.sum()
    return cells, k["used"]


def check_grid(lib, H, W, bins, rows, device="cpu", B=2, L=4.0, seed=11):
    """Grid inputs through `lib` against grid_integers with `rows`: W cells, total and count bit for bit; with whole l also the M
    cells, the ratio, iqr and valid.  -> [(ma, mb, got)] for both kinds of input."""
    out = []
    for integer in (False, True):
        ma, mb, l = grid_maps(B, H, W, bins, L, seed, integer)
        got = link_run(lib, ma, mb, device, bins=bins)
        want, _ = grid_integers(ma, mb, l, rows, bins, L, integer)
        assert np.array_equal(got[2][:, :bins], want[:, :bins]), (integer, "W cells")
        assert np.array_equal(got[2][:, 2 * bins:], want[:, 2 * bins:]), (integer, "total and count")
        if integer:
            assert np.array_equal(got[2], want), "M cells"
            for b in range(B):
                r, st, _ = orf.solve(want[b:b + 1, :bins], want[b:b + 1, bins:2 * bins], want[b:b + 1, 2 * bins] / scale_of(H, W),
                                     want[b:b + 1, 2 * bins + 1], H * W, bins, L)
                assert np.float32(r[0]) == got[0][b] and st[0, 5] == got[1][b, 5] and np.float32(st[0, 3]) == got[1][b, 3], (b, r, got[0])
        out.append((ma, mb, got))
    return out
