"""Camera trajectory from 360-degree video on the host: the emulation of pf_odo_accumulate / solve / reverse_pose
/ track / fuse (tests/emu/pf_emu_odometry.cpp compiles csrc/pf_odometry.h, the file the device kernels compile) and the Python
layer (prior_flow_amd.odometry) against the float64 restatement (tests/odometry_ref.py) under the bounds derived there; the
restatement itself against the truth of the seeded scenes; exact properties; junk; order and state; the seeded faults; the
refusals.

Figures of the restatement on the five-frame path (32x64; printed by test_five_frame_path, quoted in DESIGN.md section 22): the
worst centre error is PATH_REF and the emulation and the device are held to twice that."""
import ctypes

import numpy as np
import pytest
import torch

import egomotion_ref as er
import epipolar_cases as pc
import epipolar_ref as pr
import odometry_cases as oc
import odometry_ref as orf

bits = oc.bits


@pytest.fixture(scope="module")
def emu():
    return oc.emu()


def combos(H, W):
    """Section 20's sweep, as links: (depth, motion of pair k, motion of pair k + 1) over both depth fields, the three rotations and
    the three translations, the two baselines taken from {0.1, 0.2, 0.3} in turn (equal ones included)."""
    for depth in ("smooth", "room"):
        for r in range(3):
            for s in range(3):
                i = r * 3 + s
                T0, T1 = oc.BASELINES[i % 3], oc.BASELINES[(i + 1 + i // 3) % 3]
                yield depth, oc.motion(W, r, s, T0), oc.motion(W, r + 1, s + 1, T1)


# ---- truth -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", ((32, 64), (48, 96)))
def test_ratio_under_true_poses(emu, H, W):
    """Static scenes, the maps under the TRUE poses: the ratio is |T_k+1| / |T_k| within 1e-4, on the restatement (float64 maps) and
    on the emulation (its own maps), and the emulation's link holds the restatement's bounds on the same maps."""
    worst = [0.0, 0.0, 0.0]
    for depth, mk, mk1 in combos(H, W):
        _, bwd0, fwd1 = oc.pair_flows(H, W, mk, mk1, depth)
        truth = mk1[2] / mk[2]
        a, b = oc.true_maps(bwd0, fwd1, mk, mk1, oc.ref_mapper)
        rr, rs, _ = orf.link(a, b)
        ea, eb = oc.true_maps(bwd0, fwd1, mk, mk1, oc.lib_mapper(emu))
        got = oc.link_run(emu, ea, eb)
        for name, ratio, valid in (("restatement", rr[0], rs[0, 5]), ("emulation", got[0][0], got[1][0, 5])):
            assert valid == 1 and abs(ratio / truth - 1) <= 1e-4, (name, depth, ratio, truth)
        worst = [max(worst[0], abs(rr[0] / truth - 1)), max(worst[1], abs(got[0][0] / truth - 1)),
                 max(worst[2], oc.check_link(got, ea, eb, f"true poses {depth} {H}x{W}", cap=None)[0])]
    print(f"[odometry] true poses {H}x{W}: worst ratio error restatement {worst[0]:.2e}, emulation {worst[1]:.2e}; worst l^ error / bound {worst[2]:.2e}")


def estimated_link(lib, fwd0, bwd0, fwd1, device="cpu", **opt):
    """The link of two pairs under ESTIMATED poses through `lib`: (ratio, stats, cells, cells after), map_a, map_b."""
    e0, e1 = pc.estimate(lib, fwd0[None], device=device), pc.estimate(lib, fwd1[None], device=device)
    Rr, tr = oc.reverse_run(lib, e0["R"], e0["t"], device)
    mapper = oc.lib_mapper(lib, device)
    ma, mb = mapper(bwd0[None], Rr, tr), mapper(fwd1[None], e1["R"], e1["t"])
    return oc.link_run(lib, ma, mb, device, **opt), ma, mb


@pytest.mark.parametrize("H,W", ((32, 64), (48, 96)))
def test_ratio_under_estimated_poses(emu, H, W):
    """The 18 combinations of a size (36 over both), each pair's pose estimated from its own forward flow: within 1 %."""
    worst = 0.0
    for depth, mk, mk1 in combos(H, W):
        fwd0, bwd0, fwd1 = oc.pair_flows(H, W, mk, mk1, depth)
        got, ma, mb = estimated_link(emu, fwd0, bwd0, fwd1)
        err = abs(got[0][0] / (mk1[2] / mk[2]) - 1)
        assert got[1][0, 5] == 1 and err <= 0.01, (depth, err, got[1])
        worst = max(worst, err)
    print(f"[odometry] estimated poses {H}x{W}: worst ratio error {worst:.3%}")
    depth, mk, mk1 = next(combos(H, W))                                   # the restatement's own chain on one combination
    fwd0, bwd0, fwd1 = oc.pair_flows(H, W, mk, mk1, depth)
    ref = oc.ref_path([(fwd0[None], bwd0[None]), (fwd1[None], fwd1[None])])
    assert abs(ref[1]["ratio"][0] / (mk1[2] / mk[2]) - 1) <= 0.01 and ref[1]["link_stats"][0, 5] == 1


def robust_maps(H, W, mapper_of, moving=True):
    """Section 20's robust scene with the block moved in BOTH pairs (five columns apart in the second), poses estimated."""
    mk, mk1 = oc.motion(W, 0, 0, 0.3), oc.motion(W, 1, 1, 0.1)
    fwd0, bwd0, fwd1 = oc.pair_flows(H, W, mk, mk1, "smooth", "smooth")
    blk = pr.moved_block(H, W)
    fwd0, _ = oc.move_block(fwd0, blk)
    bwd0, _ = oc.move_block(bwd0, blk, -6.0, 2.0)
    fwd1, _ = oc.move_block(fwd1, blk, shift=5)
    return fwd0, bwd0, fwd1, 0.1 / 0.3


@pytest.mark.parametrize("H,W", ((32, 64), (48, 96)))
def test_robust_scene(emu, H, W):
    """Moved blocks in both pairs: within 0.25 % with the moving bytes, within 2 % with them zeroed; the seeded fault "mean over all
    bins" misses both caps (on the restatement, fed with the emulation's maps)."""
    fwd0, bwd0, fwd1, truth = robust_maps(H, W, None)
    got, ma, mb = estimated_link(emu, fwd0, bwd0, fwd1)
    za, zb = (ma[0], ma[1], np.zeros_like(ma[2])), (mb[0], mb[1], np.zeros_like(mb[2]))
    blind = oc.link_run(emu, za, zb)
    e1, e2 = abs(got[0][0] / truth - 1), abs(blind[0][0] / truth - 1)
    f1, f2 = (abs(orf.link(a, b, fault="mean_over_all_bins")[0][0] / truth - 1) for a, b in ((ma, mb), (za, zb)))
    r1, r2 = (abs(orf.link(a, b)[0][0] / truth - 1) for a, b in ((ma, mb), (za, zb)))
    print(f"[odometry] robust {H}x{W}: emulation {e1:.4%} (moving bytes ignored {e2:.4%}), restatement {r1:.4%} ({r2:.4%}), "
          f"mean over all bins {f1:.4%} ({f2:.4%}); moving bytes {int(ma[2].sum())} + {int(mb[2].sum())}")
    assert ma[2].any() and mb[2].any()
    assert e1 <= 0.0025 and r1 <= 0.0025 and e2 <= 0.02 and r2 <= 0.02
    assert f1 > 0.0025 and f2 > 0.02, "the seeded fault passed"
    oc.check_link(got, ma, mb, f"robust {H}x{W}")
    oc.check_link(blind, za, zb, f"robust, moving ignored {H}x{W}")


PATH_REF = {}                                                            # (H, W) -> the restatement's worst centre error


def path_errors(run, truth):
    ec_, eo = 0.0, 0.0
    for got, (A, c, S) in zip(run, truth):
        ec_ = max(ec_, float(np.linalg.norm(np.asarray(got["centre"][0], np.float64) - c)))
        eo = max(eo, er.angle_between(got["orientation"][0], A))
    return ec_, eo


def test_five_frame_path(emu):
    """Baselines 0.3, 0.1, 0.2, 0.3 over five frames at 32x64: the restatement's worst centre error is measured first, the emulation
    (Odometry.push_flows through the emulation) is held to twice that; the orientation to the sum of the pairs' R errors; the
    baselines to the links' 1 % each."""
    H, W = 32, 64
    motions = oc.path_motions(W)
    flows, truth = oc.path_flows(H, W, motions), oc.path_truth(motions)
    ref, got = oc.ref_path(flows), oc.run_path(emu, flows)
    rc, ro = path_errors(ref, truth)
    gc, go = path_errors(got, truth)
    PATH_REF[(H, W)] = rc
    r_err = sum(er.angle_between(g["pose"][0][0], m[0]) for g, m in zip(got, motions))
    print(f"[odometry] five-frame path {H}x{W}: worst centre error restatement {rc:.3e}, emulation {gc:.3e} (cap {2 * rc:.3e}) in units of the "
          f"first baseline; orientation {go:.3e} rad (sum of the R errors {r_err:.3e})")
    assert gc <= 2 * rc and go <= r_err + 8 * 4 * er.U
    for k, (g, r) in enumerate(zip(got, ref)):
        assert list(g["flags"][0]) == [k + 1, 1, 1, int(k > 0)] == list(r["flags"][0]), (k, g["flags"], r["flags"])
        assert abs(g["baseline"][0] / truth[k][2] - 1) <= 0.01 * max(k, 1), (k, g["baseline"], truth[k][2])


def test_a_pure_rotation_breaks_the_chain(emu):
    """The third of four pairs only rotates: pose valid 0, the centre stays, the orientation is still right; the pair after it opens
    segment 2 with the baseline carried."""
    H, W = 32, 64
    motions = oc.path_motions(W, still=2)
    flows = oc.path_flows(H, W, motions)
    got, ref = oc.run_path(emu, flows), oc.ref_path(flows)
    assert [list(g["flags"][0]) for g in got] == [[1, 1, 1, 0], [2, 1, 1, 1], [3, 1, 0, 0], [4, 2, 1, 0]]
    assert [list(r["flags"][0]) for r in ref] == [list(g["flags"][0]) for g in got]
    assert bits(got[2]["baseline"]).tolist() == bits(got[1]["baseline"]).tolist() == bits(got[3]["baseline"]).tolist()
    A, r_err = np.eye(3), 0.0
    for g, (R, _, _) in zip(got, motions):                               # as on the five-frame path: within the sum of the pairs' R errors
        A, r_err = R @ A, r_err + er.angle_between(g["pose"][0][0], R)
        assert er.angle_between(g["orientation"][0], A) <= r_err + 8 * 4 * er.U, "the orientation drifted"
    # the camera did not move in pair 2: the same centre (the rotation of b and of A cancel up to rounding)
    assert np.abs(got[2]["centre"] - got[1]["centre"]).max() <= 64 * er.U * max(1.0, np.abs(got[1]["centre"]).max())
    assert not got[2]["depth_weight"].any() and not got[2]["inv_depth"].any()


@pytest.mark.parametrize("H,W", ((32, 64), (48, 96)))
def test_fused_depth(emu, H, W):
    """A static scene: wherever a map counts, inv_depth S_first is |T_first| / rho within section 20's kappa sensitivity with the
    pose errors of BOTH pairs as measured on this run and the per-pixel conf, plus the measured link error (odometry_cases.
    fused_tolerance), and nothing disagrees; Odometry.push gives those bits.  The check has teeth: the seeded fault
    "fuse_wrong_scale", an all-zero depth and a depth 10 % off all fail it.  With the block moved in one pair only, every block
    pixel both maps count is flagged.  The fuse launch itself against the restatement per element."""
    s = oc.fused_scene(emu, H, W)
    inv, w, dis = s["fused"]
    tol, on, link_err = oc.fused_tolerance(s, W)
    assert on.mean() > 0.8 and np.array_equal(w[0] > 0, on) and not dis.any()
    worst = oc.fused_worst(inv, s, W)
    print(f"[odometry] fused depth {H}x{W}: worst error / tolerance {worst:.3f} (tolerance / kappa: median {np.median((tol / s['kap'])[on]):.3f}), "
          f"link error {link_err:.2e}, counted {on.mean():.1%}")
    assert worst <= 1
    fwd0, bwd0, fwd1 = s["flows"]
    pushed = oc.run_path(emu, [(fwd0[None], bwd0[None]), (fwd1[None], fwd1[None])])[1]
    assert np.array_equal(bits(pushed["inv_depth"]), bits(inv)) and np.array_equal(bits(pushed["depth_weight"]), bits(w))
    wrong = orf.fuse(s["ma"], s["mb"], s["S_a"], s["S_b"], s["lv"], fault="fuse_wrong_scale")[0]
    for name, bad in (("fuse_wrong_scale", wrong), ("all zero", np.zeros_like(inv)), ("10 % off", inv * np.float32(1.1))):
        assert oc.fused_worst(bad, s, W) > 1, (name, "passes the truth check")
    oc.check_fuse(s["fused"], s["ma"], s["mb"], s["S_a"], s["S_b"], s["lv"], f"static scene {H}x{W}")
    # the block moves in the second pair only
    m = oc.fused_scene(emu, H, W, move=True)
    ma, mb, f = m["ma"], m["mb"], m["fused"]
    oc.check_fuse(f, ma, mb, m["S_a"], m["S_b"], m["lv"], f"block in one pair {H}x{W}")
    blk = pr.moved_block(H, W)
    both = (ma[2][0] == 0) & (mb[2][0] == 0) & (ma[1][0] >= 0.05) & (mb[1][0] >= 0.05) & blk
    one = ((ma[2][0] != 0) | (ma[1][0] < 0.05)) ^ ((mb[2][0] != 0) | (mb[1][0] < 0.05))
    assert (f[2][0][both] == 1).all(), "a block pixel both maps count is not flagged"
    assert (f[2][0][blk & one] == 0).all()


# ---- equality ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", oc.SHAPES + ((40, 1100),))
@pytest.mark.parametrize("bins", (64, 512))
def test_link_matches_float64(emu, H, W, bins):
    """Batches of 1..3 scenes under estimated poses (a mask of junk kappa at B = 2): the cells, l^, ratio and iqr against the
    restatement under the derived rounding; the share of pixels near a bin edge is capped at 2 %."""
    for B in (1, 2, 3):
        if W > 1000 and B != 2:
            continue
        maps = []
        for b in range(B):
            Ta, Tb = ((0.1, 0.3), (0.3, 0.2), (0.2, 0.3))[b]                # no ratio on a bin edge (a power of two would be)
            mk, mk1 = oc.motion(W, b, b + 1, Ta), oc.motion(W, b + 1, b, Tb)
            _, bwd0, fwd1 = oc.pair_flows(H, W, mk, mk1, ("smooth", "room")[b % 2])
            maps.append(oc.true_maps(bwd0, fwd1, mk, mk1, oc.lib_mapper(emu)))
        ma = tuple(np.concatenate([m[0][i] for m in maps]) for i in range(3))
        mb = tuple(np.concatenate([m[1][i] for m in maps]) for i in range(3))
        got = oc.link_run(emu, ma, mb, bins=bins)
        oc.check_link(got, ma, mb, f"B={B} {H}x{W} bins {bins}", bins=bins)
        for b in range(B):                                               # image b of a batch gives the bits of the single-image call
            one = oc.link_run(emu, tuple(x[b:b + 1] for x in ma), tuple(x[b:b + 1] for x in mb), bins=bins)
            assert np.array_equal(one[2][0], got[2][b]) and np.array_equal(bits(one[0]), bits(got[0][b:b + 1])) \
                and np.array_equal(bits(one[1][0]), bits(got[1][b]))


@pytest.mark.parametrize("H,W", ((6, 10), (33, 70)))
@pytest.mark.parametrize("bins", (64, 512))
def test_grid_inputs_bit_for_bit(emu, H, W, bins):
    """Grid inputs (kappa_a a power of two, l at bin centres): the emulation's W cells, total and count equal the restatement's
    integers bit for bit (odometry_cases.grid_integers, with the rows of cos phi that the library itself uses), and with whole l
    also the M cells, the ratio, iqr and valid.  The rows read off pf_odo_accumulate are pf_ego_row's."""
    rows = (ctypes.c_float * H)()
    emu._dll.pf_emu_odo_rows(H, rows)
    rows = np.array(rows[:], np.float32)
    assert np.array_equal(bits(oc.rows_of(emu, H, W)), bits(rows))
    oc.check_grid(emu, H, W, bins, rows)


# ---- exact properties ------------------------------------------------------------------------------------------------------------
def some_maps(B, H, W, seed=3):
    mk, mk1 = oc.motion(W, 0, 0, 0.2), oc.motion(W, 1, 1, 0.2)
    _, bwd0, fwd1 = oc.pair_flows(H, W, mk, mk1)
    a, _ = oc.true_maps(bwd0, fwd1, mk, mk1, oc.ref_mapper)
    a = tuple(np.concatenate([x] * B) for x in a)
    rng = np.random.default_rng(seed)
    a[2][rng.random(a[2].shape) < 0.1] = 1
    return a


def test_exact_properties(emu):
    H, W, B = 33, 70, 2
    a = some_maps(B, H, W)
    ratio, stats, mid, _ = oc.link_run(emu, a, a)
    assert (bits(ratio) == bits(np.ones(B, np.float32))).all() and not stats[:, 3].any() and stats[:, 5].all() and (stats[:, 4] == 1).all()
    for j in range(-3, 4):                                               # kappa scaled by 2^j: the ratio is 2^j exactly
        b = (np.ldexp(a[0], j).astype(np.float32), a[1], a[2])
        ratio, stats, _, _ = oc.link_run(emu, a, b)
        assert (ratio == np.float32(2.0 ** j)).all() and stats[:, 5].all() and not stats[:, 3].any(), (j, ratio)
    for j in (-5, 5, 9):                                                 # beyond 2^+-L: the end bins, valid = 0
        b = (np.ldexp(a[0], j).astype(np.float32), a[1], a[2])
        ratio, stats, mid, _ = oc.link_run(emu, a, b)
        end = 0 if j < 0 else 511
        assert (ratio == 1).all() and not stats[:, 5].any() and (mid[:, end] == mid[:, 1024]).all() and mid[:, 1024].all(), j
    # everything masked
    m = (a[0], a[1], np.ones_like(a[2]))
    ratio, stats, mid, after = oc.link_run(emu, m, a)
    assert (ratio == 1).all() and not stats.any() and not mid.any() and not after.any()


def test_junk_gives_the_bits_of_moving_pixels(emu):
    """NaN, +-inf, +-1e30, negative and sub-kappa_min kappa (and junk conf) at seeded pixels: the bits of the call with those pixels
    marked moving."""
    H, W, B = 33, 70, 2
    a = some_maps(B, H, W)
    b = (np.ldexp(a[0], 1).astype(np.float32), a[1].copy(), np.zeros_like(a[2]))
    rng = np.random.default_rng(8)
    bad = rng.random(a[0].shape) < 0.1
    junk = rng.choice(np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, -0.5, 5e-5, 0.0], np.float32), size=a[0].shape)
    which = rng.integers(0, 3, a[0].shape)
    ja = (np.where(bad & (which == 0), junk, a[0]), a[1], a[2])
    jb = (np.where(bad & (which == 1), junk, b[0]), np.where(bad & (which == 2), np.minimum(junk, 0), b[1]).astype(np.float32), b[2])
    clean_b = (b[0], b[1], bad.astype(np.uint8))
    got, want = oc.link_run(emu, ja, jb), oc.link_run(emu, a, clean_b)
    assert want[2].any() and all(np.array_equal(bits(x), bits(y)) for x, y in zip(got, want))
    S = np.array([1.0, 0.5], np.float32)
    f1, f2 = oc.fuse_run(emu, ja, jb, S, S, np.ones(B)), oc.fuse_run(emu, (a[0], a[1], a[2] | (bad & (which == 0))), (b[0], b[1], (bad & (which > 0)).astype(np.uint8)), S, S, np.ones(B))
    zero_ok = bad & (((which == 0) & (junk == 0)) | ((which == 1) & (junk == 0)) | ((which == 0) & (junk == np.float32(5e-5))) | ((which == 1) & (junk == np.float32(5e-5))))
    assert all(np.array_equal(bits(x)[~zero_ok], bits(y)[~zero_ok]) for x, y in zip(f1, f2))     # 0 <= kappa < kappa_min counts in the fuse


# ---- order and state -------------------------------------------------------------------------------------------------------------
def test_order_and_leftovers(emu):
    H, W, B = 33, 70, 3
    a = some_maps(B, H, W)
    b = (np.ldexp(a[0], -1).astype(np.float32) * np.float32(1.01), a[1], np.zeros_like(a[2]))
    want = oc.link_run(emu, a, b)
    try:
        for order in (1, 12345, 99):
            emu._dll.pf_emu_odo_order(order)
            got = oc.link_run(emu, a, b)
            assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(got, want)), order
    finally:
        emu._dll.pf_emu_odo_order(0)
    assert not want[3].any(), "the solve left cells behind"


def test_poisoned_state_and_reset(emu):
    """Histograms, state and outputs poisoned with NaN / +-1e30 bit patterns before reset() give the bits of a fresh object."""
    from prior_flow_amd.odometry import Odometry
    H, W = 32, 64
    flows = oc.path_flows(H, W, oc.path_motions(W)[:3])
    fresh = oc.run_path(emu, flows)
    for junk, isum in ((float("nan"), 0x7FF8123456789ABC), (1e30, 2 ** 62), (-1e30, -2 ** 62)):
        odo = Odometry(1, H, W, "cpu", lib=emu)
        oc.run_path(emu, flows[:2], odo=odo)
        for buf in (odo.state, odo.orientation, odo.centre, odo.baseline, odo.prev_baseline, odo.link_valid, odo.ratio, odo.link_stats,
                    odo.inv_depth, odo.depth_weight, odo.R_rev, odo.t_rev, odo.pose.R, odo.pose.t, odo.pose.stats) + odo.map_a[:3] + odo.map_b[:3]:
            buf.fill_(junk)
        for buf in (odo.flags, odo.disagree, odo.map_a[3], odo.map_b[3]):
            buf.fill_(77)
        odo.scale.hist.fill_(isum)
        odo.pose.sums.fill_(isum)
        odo.reset()
        got = oc.run_path(emu, flows, odo=odo)
        for g, f in zip(got, fresh):
            assert all(np.array_equal(bits(g[k]), bits(f[k])) for k in f if k != "pose"), junk


@pytest.mark.parametrize("W", (4096, 4097))
def test_worst_case_row_does_not_overflow(emu, W):
    """Every pixel of a row in ONE bin at w = 1, l_c = L: n 2^S stays at or below 2^62, at a power of two and one past it."""
    out = (ctypes.c_longlong * 2)()
    emu._dll.pf_emu_odo_worst(1, W, out)
    lg = int(np.ceil(np.log2(W)))
    assert out[0] == out[1] == W << (62 - lg) and 0 < out[0] <= 1 << 62


# ---- track, reverse pose, fuse against float64 -------------------------------------------------------------------------------------
def test_track_and_reverse_match_float64(emu):
    """Twelve steps of three chains with seeded valid flags and ratios: orientation, centre and baseline within 8 U per step (of the
    value's size), the flags exactly; the reversed pose within 8 U, R^T bit for bit, t = 0 gives +0."""
    B, n = 3, 12
    rng = np.random.default_rng(4)
    run, ref = oc.TrackRun(emu, B), orf.Track(B)
    for k in range(n):
        R = np.stack([er.axis_angle(rng.normal(size=3), rng.uniform(0, 40)) for _ in range(B)]).astype(np.float32)
        t = np.stack([pr.unit(rng.normal(size=3)) for _ in range(B)]).astype(np.float32)
        pv, lv = rng.random(B) < 0.8, rng.random(B) < 0.8
        ratio = np.exp2(rng.uniform(-1, 1, B)).astype(np.float32)
        t[~pv] = 0
        go, gc, gs, gf = run.step(R, t, pv, ratio, lv)
        ro, rc, rs, rf = ref.step(R, t, pv, ratio, lv)
        size = max(1.0, float(np.abs(rc).max()))
        assert np.array_equal(gf, rf), (k, gf, rf)
        assert np.abs(go - ro).max() <= 8 * er.U * (k + 1) and np.abs(gc - rc).max() <= 8 * er.U * (k + 1) * size, k
        assert (np.abs(gs / rs - 1) <= 8 * er.U * (k + 1)).all()
        Rr, tr = oc.reverse_run(emu, R, t)
        wR, wt = orf.reverse_pose(R, t)
        assert np.array_equal(bits(Rr), bits(np.ascontiguousarray(R.transpose(0, 2, 1)))) and np.abs(tr - wt).max() <= 8 * er.U
        assert not np.signbit(tr[~pv]).any() and not tr[~pv].any()


def test_fuse_matches_float64(emu):
    H, W, B = 33, 70, 2
    a = some_maps(B, H, W)
    rng = np.random.default_rng(6)
    b = ((a[0] * np.exp2(rng.normal(0, 0.4, a[0].shape))).astype(np.float32), rng.random(a[1].shape).astype(np.float32), (rng.random(a[2].shape) < 0.1).astype(np.uint8))
    for S_a, S_b, lv in (((1.0, 0.5), (0.7, 2.0), (1, 1)), ((1.0, 1.0), (1.0, 1.0), (1, 0))):
        got = oc.fuse_run(emu, a, b, S_a, S_b, lv)
        oc.check_fuse(got, a, b, S_a, S_b, np.asarray(lv), f"fuse lv={lv}")
        if lv[1] == 0:
            alone = np.where((b[2][1] == 0) & (b[1][1] >= np.float32(0.05)) & (b[0][1] >= 0), b[0][1], np.float32(0))
            assert (np.abs(got[0][1] - alone) <= 2 * er.U * alone).all(), "without a valid link only map b counts"
            assert not got[2][1].any()
    weightless(emu, a, b)


def weightless(lib, a, b, device="cpu"):
    """conf_min = 0 with conf = 0 in both maps, and conf = +inf: the weight sum is 0 or infinite, nothing counts, the outputs are
    zeros and never 0 / 0 or inf / inf."""
    rng = np.random.default_rng(9)
    zero, inf = rng.random(a[0].shape) < 0.2, rng.random(a[0].shape) < 0.1
    ca = np.where(zero, np.float32(0), np.where(inf, np.float32(np.inf), a[1])).astype(np.float32)
    cb = np.where(zero, np.float32(0), b[1]).astype(np.float32)
    ja, jb = (a[0], ca, a[2]), (b[0], cb, b[2])
    got = oc.fuse_run(lib, ja, jb, (1.0, 0.5), (0.7, 2.0), (1, 1), device, conf_min=0.0)
    oc.check_fuse(got, ja, jb, (1.0, 0.5), (0.7, 2.0), np.ones(2), "fuse with weight sums of 0 and inf", conf_min=0.0)
    gone = zero | (inf & (a[2] == 0))
    assert gone.any() and not got[0][gone].any() and not got[1][gone].any()


# ---- teeth -------------------------------------------------------------------------------------------------------------------------
def test_every_seeded_fault_is_caught(emu):
    """Each deliberate mistake of odometry_ref.FAULTS, built into the restatement, fails a named check of this file that the correct
    restatement passes."""
    H, W = 32, 64
    caught = {}
    # the robust scene's maps (from the emulation): faults of the link
    fwd0, bwd0, fwd1, truth = robust_maps(H, W, None)
    got, ma, mb = estimated_link(emu, fwd0, bwd0, fwd1)

    def link_ok(fault, a=ma, b=mb, cap=0.0025, want=truth):
        r, s, _ = orf.link(a, b, fault=fault)
        return s[0, 5] == 1 and abs(r[0] / want - 1) <= cap

    def cells_ok(fault):
        try:
            k = orf.link_terms(ma, mb, fault=fault)
            Wh = orf.histogram(k, 512, 4.0)[0]
            return np.abs(got[2][0, :512] * oc.er_scale_inv(H, W) - Wh[0]).sum() <= 0.02 * Wh.sum()
        except AssertionError:
            return False

    assert link_ok(None) and cells_ok(None)
    caught["no_cos_weight"] = not cells_ok("no_cos_weight")                              # test_link_matches_float64's cells
    caught["moving_ignored"] = not cells_ok("moving_ignored")
    caught["ratio_inverted"] = not link_ok("ratio_inverted")                             # test_ratio_under_*_poses
    caught["mean_over_all_bins"] = not link_ok("mean_over_all_bins")                     # test_robust_scene
    # ratios beyond 2^L: test_exact_properties' end bins
    a = some_maps(1, H, W)
    far = (np.ldexp(a[0], 5).astype(np.float32), a[1], a[2])
    assert orf.link(a, far)[1][0, 5] == 0
    caught["clamp_bins_valid"] = orf.link(a, far, fault="clamp_bins_valid")[1][0, 5] != 0
    # a median two bins above the lower end: the cut window against the emulation
    top = np.random.default_rng(2).random(a[0].shape) < 0.2              # a fifth of the pixels just below the upper end
    near_end = (np.where(top, np.ldexp(a[0], 4) * np.float32(0.985), np.ldexp(a[0], -4) * np.float32(1.03)).astype(np.float32), a[1], a[2])
    e = oc.link_run(emu, a, near_end)
    good, bad = orf.link(a, near_end), orf.link(a, near_end, fault="window_not_cut")
    assert good[2]["info"][0]["m"] in (1, 2, 3) and abs(good[1][0, 2] - e[1][0, 2]) <= 1e-5
    caught["window_not_cut"] = abs(bad[1][0, 2] - e[1][0, 2]) > 1e-5
    # the chain: test_a_pure_rotation_breaks_the_chain's carried baseline, test_five_frame_path's centres
    motions = oc.path_motions(W, still=2)
    flows = oc.path_flows(H, W, motions)
    ok, f7 = oc.ref_path(flows), oc.ref_path(flows, fault="scale_before_validity")
    assert ok[2]["baseline"][0] == ok[1]["baseline"][0]
    assert f7[2]["baseline"][0] == f7[1]["baseline"][0]                   # an invalid link reports ratio 1: the path does not notice,
    run, good, bad = oc.TrackRun(emu, 1), orf.Track(1), orf.Track(1, "scale_before_validity")      # test_track_and_reverse_match_float64 does
    Rk, tk = motions[0][0][None], motions[0][1][None]
    for pv, lv in ((1, 1), (1, 0), (0, 1), (1, 1)):
        gs = run.step(Rk, tk, [pv], [2.0], [lv])[2]
        ws, bs = good.step(Rk, tk, [pv], [2.0], [lv])[2], bad.step(Rk, tk, [pv], [2.0], [lv])[2]
    assert gs[0] == ws[0] == 1.0
    caught["scale_before_validity"] = bs[0] != gs[0]
    motions = oc.path_motions(W)
    flows, truth_p = oc.path_flows(H, W, motions), oc.path_truth(motions)
    rc = path_errors(oc.ref_path(flows), truth_p)[0]
    caught["b_not_rotated"] = path_errors(oc.ref_path(flows, fault="b_not_rotated"), truth_p)[0] > 2 * rc
    # the fuse: test_fuse_matches_float64
    b = (np.ldexp(a[0], -1).astype(np.float32), a[1], a[2])
    gotf = oc.fuse_run(emu, a, b, (1.0,), (0.5,), (1,))
    oc.check_fuse(gotf, a, b, (1.0,), (0.5,), np.ones(1), "fuse for the teeth")
    try:
        rinv = orf.fuse(a, b, np.ones(1), np.full(1, 0.5), np.ones(1), fault="fuse_wrong_scale")[0]
        caught["fuse_wrong_scale"] = bool((np.abs(gotf[0] - rinv) > 6 * orf.U * np.maximum(rinv, 1)).any())
    except AssertionError:
        caught["fuse_wrong_scale"] = True
    assert set(caught) == set(orf.FAULTS) and all(caught.values()), caught


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals(emu):
    """Each rule of the *_check functions once, through the emulation (the checks are the header's): -1 = PF_ERR_BAD_ARG, -2 =
    PF_ERR_BAD_SHAPE."""
    d = emu._dll
    B, H, W, bins = 1, 4, 8, 64
    N = H * W
    f = [torch.zeros(N) for _ in range(6)]
    u = [torch.zeros(N, dtype=torch.uint8) for _ in range(3)]
    hist = torch.zeros(2 * bins + 2, dtype=torch.int64)
    p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())   # noqa: E731

    def acc(a=(f[0], f[1], u[0]), b=(f[2], f[3], u[1]), h=hist, B=B, H=H, W=W, bins=bins, L=4.0, kmin=1e-4, blocks=0, off=0):
        hp = None if h is None else ctypes.c_void_p(h.data_ptr() + off)
        return d.pf_odo_accumulate(p(a[0]), p(a[1]), p(a[2]), p(b[0]), p(b[1]), p(b[2]), hp, B, H, W, bins, L, kmin, blocks, None)

    assert acc() == 0
    assert acc(a=(None, f[1], u[0])) == -1 and acc(b=(f[2], f[3], None)) == -1 and acc(h=None) == -1 and acc(off=4) == -1
    assert acc(bins=32) == -1 and acc(bins=96) == -1 and acc(bins=2048) == -1
    assert acc(L=0.0) == -1 and acc(L=float("inf")) == -1 and acc(L=float("nan")) == -1 and acc(kmin=0.0) == -1 and acc(kmin=-1.0) == -1
    assert acc(blocks=-1) == -1 and acc(blocks=65536) == -1
    assert acc(B=0) == -2 and acc(H=0) == -2 and acc(H=1 << 15, W=1 << 15) == -2
    big = torch.zeros(N + 2 * (2 * bins + 2))
    assert d.pf_odo_accumulate(p(big), p(f[1]), p(u[0]), p(f[2]), p(f[3]), p(u[1]), ctypes.c_void_p(big.data_ptr() + 4 * N - 8), B, H, W,
                               bins, 4.0, 1e-4, 0, None) == -1         # the cells meet an input's last bytes
    assert d.pf_odo_hist_bytes(1, H, W, bins) == (2 * bins + 2) * 8 and d.pf_odo_hist_bytes(1, H, W, 100) == -1 and d.pf_odo_hist_bytes(0, H, W, bins) == -2
    ratio, stats = torch.zeros(1), torch.zeros(6)

    def solve(h=hist, r=ratio, s=stats, B=B, bins=bins, L=4.0, trim=4, mu=0.05, iqr=1.0):
        return d.pf_odo_solve(p(h), p(r), p(s), B, H, W, bins, L, trim, mu, iqr, None)

    assert solve() == 0
    assert solve(h=None) == -1 and solve(r=None) == -1 and solve(s=None) == -1 and solve(r=stats) == -1
    assert solve(bins=65) == -1 and solve(L=-1.0) == -1 and solve(trim=-1) == -1 and solve(mu=-0.1) == -1 and solve(mu=float("nan")) == -1
    assert solve(iqr=0.0) == -1 and solve(iqr=float("inf")) == -1 and solve(B=0) == -2
    R, t, Rr, tr = torch.eye(3).reshape(1, 9).contiguous(), torch.zeros(3), torch.zeros(9), torch.zeros(3)
    assert d.pf_odo_reverse_pose(p(R), p(t), p(Rr), p(tr), 1, None) == 0
    assert d.pf_odo_reverse_pose(p(R), p(t), p(R), p(tr), 1, None) == -1 and d.pf_odo_reverse_pose(p(R), p(t), p(Rr), p(t), 1, None) == -1
    assert d.pf_odo_reverse_pose(None, p(t), p(Rr), p(tr), 1, None) == -1 and d.pf_odo_reverse_pose(p(R), p(t), p(Rr), p(tr), 0, None) == -2
    ps, ls, rat = torch.zeros(6), torch.zeros(6), torch.ones(1)
    state, orient, centre, base, flags = torch.zeros(12, dtype=torch.float64), torch.zeros(9), torch.zeros(3), torch.zeros(1), torch.zeros(4, dtype=torch.int32)

    def track(**kw):
        a = dict(R=R, t=t, ps=ps, rat=rat, ls=ls, state=state, orient=orient, centre=centre, base=base, flags=flags)
        a.update(kw)
        return d.pf_odo_track(*(p(a[k]) for k in ("R", "t", "ps", "rat", "ls", "state", "orient", "centre", "base", "flags")), kw.get("B", 1), None)

    assert track() == 0
    for k in ("R", "t", "ps", "rat", "ls", "state", "orient", "centre", "base", "flags"):
        assert track(**{k: None}) == -1, k
    assert track(orient=R) == -1 and track(centre=t) == -1 and track(base=rat) == -1 and track(B=0) == -2
    S = torch.ones(1)
    outs = [torch.zeros(N), torch.zeros(N), torch.zeros(N, dtype=torch.uint8)]

    def fz(a=(f[0], f[1], u[0]), b=(f[2], f[3], u[1]), Sa=S, Sb=S, lv=rat, o=outs, cm=0.05, kmin=1e-4, tol=0.5, B=B):
        return d.pf_odo_fuse(p(a[0]), p(a[1]), p(a[2]), p(b[0]), p(b[1]), p(b[2]), p(Sa), p(Sb), p(lv), p(o[0]), p(o[1]), p(o[2]), B, H, W,
                             cm, kmin, tol, None)

    assert fz() == 0 and fz(o=[None, None, None]) == 0
    assert fz(a=(None, f[1], u[0])) == -1 and fz(Sa=None) == -1 and fz(lv=None) == -1
    assert fz(o=[f[0], outs[1], outs[2]]) == -1 and fz(o=[outs[0], outs[0], outs[2]]) == -1 and fz(o=[outs[0], outs[1], u[1]]) == -1
    assert fz(cm=-1.0) == -1 and fz(kmin=0.0) == -1 and fz(tol=0.0) == -1 and fz(tol=float("nan")) == -1 and fz(B=0) == -2


def test_python_layer_refuses_host_tensors_and_bad_options(emu):
    from prior_flow_amd._lib import PfError
    from prior_flow_amd.odometry import Odometry, ScaleLink, fuse_depth
    B, H, W = 1, 8, 16
    for bad in (lambda: ScaleLink(B, H, W, "cpu"), lambda: Odometry(B, H, W, "cpu"), lambda: ScaleLink(B, H, W, "cpu", lib=emu, bins=100),
                lambda: ScaleLink(B, H, W, "cpu", lib=emu, trim_bins=-1), lambda: ScaleLink(B, H, W, "cpu", lib=emu, log2_range=0),
                lambda: Odometry(B, H, W, "cpu", lib=emu, nonsense=1), lambda: Odometry(B, H, W, "cpu", lib=emu).push(None),
                lambda: fuse_depth((torch.zeros(B, H, W),) * 3, (torch.zeros(B, H, W),) * 3, torch.ones(B), torch.ones(B), torch.ones(B)),
                lambda: ScaleLink(B, H, W, "cpu", lib=emu).link((torch.zeros(B, H, W),) * 3, (torch.zeros(B, H, W),) * 3)):
        with pytest.raises(PfError):
            bad()
