"""Camera trajectory from 360-degree video on an MI355X: pf_odo_accumulate, pf_odo_solve, pf_odo_reverse_pose,
pf_odo_track and pf_odo_fuse on the device through the checks of tests/test_odometry_host.py -- the float64 restatement
(tests/odometry_ref.py) under the bounds derived there, the truth of the seeded scenes, the exact properties -- and against the
host emulation of the same header; reproducibility under repeated calls and other grids; poisoned buffers; the Python layer
(prior_flow_amd.odometry), eager and captured, behind a bidirectional FlowStream.  Run with ``-m gpu``.

The device and the emulation are NOT bit for bit the same on the cells: cos phi of a row is cosf of two libraries (as in section
20), so a cell may differ by the rounding of the weight.  What is integer on both sides (the count, which bins are occupied, valid)
is compared exactly, the cells within that rounding, and whether every cell happened to agree is printed."""
import argparse

import numpy as np
import pytest
import torch

import egomotion_ref as er
import epipolar_cases as pc
import epipolar_ref as pr
import golden_cases as gc
import odometry_cases as oc
import odometry_ref as orf
import test_odometry_host as th

pytestmark = pytest.mark.gpu
bits = oc.bits
DEV = "cuda"


@pytest.fixture(scope="module")
def emu():
    return oc.emu()


@pytest.fixture(scope="module")
def lib():
    from prior_flow_amd._lib import load
    return load()


def same(a, b):
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def against_emulation(got, want, ma, mb, bins, what):
    """A device link against the emulation's on the same maps: integers exactly, cells within the rounding of cos phi (W_ABS for
    either side) plus the weight of the pixels whose l lies within the rounding of a bin edge, where the two log2f may part."""
    B, H, W = ma[0].shape
    inv = oc.er_scale_inv(H, W)
    k = orf.link_terms(ma, mb, bins, 4.0)
    assert np.array_equal(got[2][:, 2 * bins + 1], want[2][:, 2 * bins + 1]), (what, "count")
    equal = np.array_equal(got[2], want[2])
    for b in range(B):
        n = float(got[2][b, 2 * bins + 1])
        for lo in (0, bins):
            d = np.abs((got[2][b, lo:lo + bins] - want[2][b, lo:lo + bins]).astype(np.float64)) * inv
            near = 2 * float(k["w"][b][k["near"][b]].sum())
            assert d.sum() <= 2 * orf.W_ABS * n + near + 2 * orf.edge_rounding(4.0) * n, (what, b, "cells", d.sum())
    print(f"[odometry] {what}: device cells {'equal' if equal else 'differ from'} the emulation's bit for bit")
    return equal


@pytest.mark.parametrize("H,W", oc.SHAPES + ((40, 1100),))
@pytest.mark.parametrize("bins", (64, 512))
def test_device_link_matches_float64_and_the_emulation(lib, emu, H, W, bins):
    """test_link_matches_float64's batches on the device: the cells, l^, ratio and iqr against the restatement under the derived
    rounding, image b of a batch against the single-image call, and the emulation on the same maps."""
    for B in (1, 2, 3):
        if W > 1000 and B != 2:
            continue
        maps = []
        for b in range(B):
            Ta, Tb = ((0.1, 0.3), (0.3, 0.2), (0.2, 0.3))[b]
            mk, mk1 = oc.motion(W, b, b + 1, Ta), oc.motion(W, b + 1, b, Tb)
            _, bwd0, fwd1 = oc.pair_flows(H, W, mk, mk1, ("smooth", "room")[b % 2])
            maps.append(oc.true_maps(bwd0, fwd1, mk, mk1, oc.lib_mapper(lib, DEV)))
        ma = tuple(np.concatenate([m[0][i] for m in maps]) for i in range(3))
        mb = tuple(np.concatenate([m[1][i] for m in maps]) for i in range(3))
        got = oc.link_run(lib, ma, mb, DEV, bins=bins)
        oc.check_link(got, ma, mb, f"device B={B} {H}x{W} bins {bins}", bins=bins)
        for b in range(B):
            one = oc.link_run(lib, tuple(x[b:b + 1] for x in ma), tuple(x[b:b + 1] for x in mb), DEV, bins=bins)
            assert np.array_equal(one[2][0], got[2][b]) and np.array_equal(bits(one[0]), bits(got[0][b:b + 1])) \
                and np.array_equal(bits(one[1][0]), bits(got[1][b]))
        against_emulation(got, oc.link_run(emu, ma, mb, bins=bins), ma, mb, bins, f"B={B} {H}x{W} bins {bins}")


@pytest.mark.parametrize("H,W", ((32, 64), (48, 96)))
def test_device_against_the_truth(lib, H, W):
    """True poses within 1e-4 and estimated poses within 1 % over the 18 combinations of a size; the robust scene within 0.25 % with
    the moving bytes and 2 % without, where the seeded fault "mean over all bins" misses both caps."""
    worst = [0.0, 0.0]
    for depth, mk, mk1 in th.combos(H, W):
        fwd0, bwd0, fwd1 = oc.pair_flows(H, W, mk, mk1, depth)
        truth = mk1[2] / mk[2]
        ea, eb = oc.true_maps(bwd0, fwd1, mk, mk1, oc.lib_mapper(lib, DEV))
        got = oc.link_run(lib, ea, eb, DEV)
        assert got[1][0, 5] == 1 and abs(got[0][0] / truth - 1) <= 1e-4, (depth, got[0], truth)
        est, _, _ = th.estimated_link(lib, fwd0, bwd0, fwd1, DEV)
        assert est[1][0, 5] == 1 and abs(est[0][0] / truth - 1) <= 0.01, (depth, est[0], truth)
        worst = [max(worst[0], abs(got[0][0] / truth - 1)), max(worst[1], abs(est[0][0] / truth - 1))]
    print(f"[odometry] device {H}x{W}: worst ratio error under true poses {worst[0]:.2e}, under estimated poses {worst[1]:.3%}")
    fwd0, bwd0, fwd1, truth = th.robust_maps(H, W, None)
    got, ma, mb = th.estimated_link(lib, fwd0, bwd0, fwd1, DEV)
    za, zb = (ma[0], ma[1], np.zeros_like(ma[2])), (mb[0], mb[1], np.zeros_like(mb[2]))
    blind = oc.link_run(lib, za, zb, DEV)
    e1, e2 = abs(got[0][0] / truth - 1), abs(blind[0][0] / truth - 1)
    f1, f2 = (abs(orf.link(a, b, fault="mean_over_all_bins")[0][0] / truth - 1) for a, b in ((ma, mb), (za, zb)))
    print(f"[odometry] device robust {H}x{W}: {e1:.4%} (moving bytes ignored {e2:.4%}); mean over all bins {f1:.4%} ({f2:.4%})")
    assert e1 <= 0.0025 and e2 <= 0.02 and f1 > 0.0025 and f2 > 0.02
    oc.check_link(got, ma, mb, f"device robust {H}x{W}")


def test_device_paths(lib):
    """The five-frame path: centres within twice the restatement's worst error, the orientation within the sum of the pairs' R errors;
    a pure rotation in the middle opens a new segment with the baseline carried."""
    H, W = 32, 64
    motions = oc.path_motions(W)
    flows, truth = oc.path_flows(H, W, motions), oc.path_truth(motions)
    rc, _ = th.path_errors(oc.ref_path(flows), truth)
    got = oc.run_path(lib, flows, DEV)
    gc_, go = th.path_errors(got, truth)
    r_err = sum(er.angle_between(g["pose"][0][0], m[0]) for g, m in zip(got, motions))
    print(f"[odometry] device five-frame path {H}x{W}: worst centre error {gc_:.3e} (restatement {rc:.3e}, cap {2 * rc:.3e}); orientation "
          f"{go:.3e} rad (sum of the R errors {r_err:.3e})")
    assert gc_ <= 2 * rc and go <= r_err + 8 * 4 * er.U
    assert [list(g["flags"][0]) for g in got] == [[k + 1, 1, 1, int(k > 0)] for k in range(4)]
    for k, g in enumerate(got):
        assert abs(g["baseline"][0] / truth[k][2] - 1) <= 0.01 * max(k, 1)
    motions = oc.path_motions(W, still=2)
    got = oc.run_path(lib, oc.path_flows(H, W, motions), DEV)
    assert [list(g["flags"][0]) for g in got] == [[1, 1, 1, 0], [2, 1, 1, 1], [3, 1, 0, 0], [4, 2, 1, 0]]
    assert bits(got[2]["baseline"]).tolist() == bits(got[1]["baseline"]).tolist() == bits(got[3]["baseline"]).tolist()
    A, r_err = np.eye(3), 0.0
    for g, (R, _, _) in zip(got, motions):                               # as on the five-frame path: within the sum of the pairs' R errors
        A, r_err = R @ A, r_err + er.angle_between(g["pose"][0][0], R)
        assert er.angle_between(g["orientation"][0], A) <= r_err + 8 * 4 * er.U
    assert not got[2]["depth_weight"].any() and not got[2]["inv_depth"].any()


@pytest.mark.parametrize("H,W", ((32, 64), (48, 96)))
def test_device_fused_depth(lib, H, W):
    """test_fused_depth on the device: the static scene's depth in trajectory units within section 20's sensitivity under the pose
    errors measured on this run and the measured link error, nothing disagrees, Odometry.push gives those bits, and a wrong scale,
    an all-zero depth and a depth 10 % off fail the check; the block moved in one pair only is flagged; the fuse launch against the
    restatement per element."""
    s = oc.fused_scene(lib, H, W, DEV)
    inv, w, dis = s["fused"]
    tol, on, link_err = oc.fused_tolerance(s, W)
    assert on.mean() > 0.8 and np.array_equal(w[0] > 0, on) and not dis.any()
    worst = oc.fused_worst(inv, s, W)
    print(f"[odometry] device fused depth {H}x{W}: worst error / tolerance {worst:.3f}, link error {link_err:.2e}, counted {on.mean():.1%}")
    assert worst <= 1
    fwd0, bwd0, fwd1 = s["flows"]
    pushed = oc.run_path(lib, [(fwd0[None], bwd0[None]), (fwd1[None], fwd1[None])], DEV)[1]
    assert np.array_equal(bits(pushed["inv_depth"]), bits(inv)) and np.array_equal(bits(pushed["depth_weight"]), bits(w))
    wrong = orf.fuse(s["ma"], s["mb"], s["S_a"], s["S_b"], s["lv"], fault="fuse_wrong_scale")[0]
    for name, bad in (("fuse_wrong_scale", wrong), ("all zero", np.zeros_like(inv)), ("10 % off", inv * np.float32(1.1))):
        assert oc.fused_worst(bad, s, W) > 1, (name, "passes the truth check")
    oc.check_fuse(s["fused"], s["ma"], s["mb"], s["S_a"], s["S_b"], s["lv"], f"device static scene {H}x{W}")
    m = oc.fused_scene(lib, H, W, DEV, move=True)
    ma, mb, f = m["ma"], m["mb"], m["fused"]
    oc.check_fuse(f, ma, mb, m["S_a"], m["S_b"], m["lv"], f"device block in one pair {H}x{W}")
    both = (ma[2][0] == 0) & (mb[2][0] == 0) & (ma[1][0] >= 0.05) & (mb[1][0] >= 0.05) & pr.moved_block(H, W)
    assert (f[2][0][both] == 1).all()


@pytest.mark.parametrize("H,W", ((6, 10), (33, 70)))
@pytest.mark.parametrize("bins", (64, 512))
def test_device_grid_inputs_bit_for_bit(lib, emu, H, W, bins):
    """Grid inputs on the device against the restatement's integers (odometry_cases.grid_integers) built with the DEVICE's rows of
    cos phi, which are read off pf_odo_accumulate itself (one used pixel per row): W cells, total and count bit for bit, and with
    whole l also the M cells, the ratio, iqr and valid.  Then device against emulation bit for bit, on the rows where the two cosf
    agree (the others are marked moving for both): every cell, ratio and stats with whole l; with l at bin centres the W cells,
    total and count (there the M cells carry log2f of two libraries, which no rule makes equal)."""
    import ctypes
    rows = oc.rows_of(lib, H, W, DEV)
    assert (np.abs(rows.astype(np.float64) - orf.cos_rows(H)) <= orf.W_ABS).all()
    runs = oc.check_grid(lib, H, W, bins, rows, DEV)
    host = (ctypes.c_float * H)()
    emu._dll.pf_emu_odo_rows(H, host)
    agree = bits(np.array(host[:], np.float32)) == bits(rows)
    print(f"[odometry] grid inputs {H}x{W} bins {bins}: the device's and the emulation's cos phi agree on {int(agree.sum())} of {H} rows")
    for integer, (ma, mb, _) in zip((False, True), runs):
        mv = ma[2] | (~agree)[None, :, None].astype(np.uint8)
        ma = (ma[0], ma[1], mv)
        d, e = oc.link_run(lib, ma, mb, DEV, bins=bins), oc.link_run(emu, ma, mb, bins=bins)
        assert np.array_equal(d[2][:, :bins], e[2][:, :bins]) and np.array_equal(d[2][:, 2 * bins:], e[2][:, 2 * bins:]), integer
        if integer:
            assert same(d, e)


def test_device_exact_properties_and_junk(lib):
    H, W, B = 33, 70, 2
    a = th.some_maps(B, H, W)
    ratio, stats, _, _ = oc.link_run(lib, a, a, DEV)
    assert (bits(ratio) == bits(np.ones(B, np.float32))).all() and not stats[:, 3].any() and stats[:, 5].all()
    for j in range(-3, 4):
        ratio, stats, _, _ = oc.link_run(lib, a, (np.ldexp(a[0], j).astype(np.float32), a[1], a[2]), DEV)
        assert (ratio == np.float32(2.0 ** j)).all() and stats[:, 5].all() and not stats[:, 3].any(), (j, ratio)
    for j in (-5, 5, 9):
        ratio, stats, mid, _ = oc.link_run(lib, a, (np.ldexp(a[0], j).astype(np.float32), a[1], a[2]), DEV)
        assert (ratio == 1).all() and not stats[:, 5].any() and (mid[:, 0 if j < 0 else 511] == mid[:, 1024]).all() and mid[:, 1024].all(), j
    ratio, stats, mid, after = oc.link_run(lib, (a[0], a[1], np.ones_like(a[2])), a, DEV)
    assert (ratio == 1).all() and not stats.any() and not mid.any() and not after.any()
    # junk at seeded pixels gives the bits of the call with those pixels marked moving
    b = (np.ldexp(a[0], 1).astype(np.float32), a[1].copy(), np.zeros_like(a[2]))
    rng = np.random.default_rng(8)
    bad = rng.random(a[0].shape) < 0.1
    junk = rng.choice(np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, -0.5, 5e-5, 0.0], np.float32), size=a[0].shape)
    which = rng.integers(0, 3, a[0].shape)
    ja = (np.where(bad & (which == 0), junk, a[0]), a[1], a[2])
    jb = (np.where(bad & (which == 1), junk, b[0]), np.where(bad & (which == 2), np.minimum(junk, 0), b[1]).astype(np.float32), b[2])
    want = oc.link_run(lib, a, (b[0], b[1], bad.astype(np.uint8)), DEV)
    assert want[2].any() and same(oc.link_run(lib, ja, jb, DEV), want)


@pytest.mark.parametrize("bins", (64, 512))
def test_same_bits_on_every_run_and_for_every_grid(lib, emu, bins):
    """Two runs, and grids of 1, 3 and 64 workgroups per image against the one chosen from the CU count, on a concentrated input
    (a static scene: one or two bins, the wave-combined path), a spread one (grid inputs: the lane-by-lane path) and a half-and-half
    mix: the same cells, ratio and stats.  33x70 on one workgroup is 33 strips for 16 waves and 40x1100 nine strips to a row, the
    last one ragged.  The grid inputs also against the emulation."""
    for (H, W), B in (((33, 70), 3), ((40, 1100), 2), ((6, 10), 1)):
        a = th.some_maps(B, H, W)
        conc = (a, (np.ldexp(a[0], 1).astype(np.float32) * np.float32(1.003), a[1], np.zeros_like(a[2])))
        ga, gb, _ = oc.grid_maps(B, H, W, bins, 4.0, 5)
        mix = np.random.default_rng(1).random(a[0].shape) < 0.5
        mixed = (tuple(np.where(mix, x, y) for x, y in zip(conc[0], ga)), tuple(np.where(mix, x, y) for x, y in zip(conc[1], gb)))
        for name, (ma, mb) in (("concentrated", conc), ("spread", (ga, gb)), ("mixed", mixed)):
            want = None
            for blocks in (0, 0, 1, 3, 64):
                got = oc.link_run(lib, ma, mb, DEV, blocks=blocks, bins=bins)
                assert got[2].any()
                want = got if want is None else want
                assert same(got, want), ((H, W), name, blocks)
            e = oc.link_run(emu, ma, mb, bins=bins)
            occupied = lambda g: g[2][:, :bins] != 0                     # noqa: E731
            if name == "spread":
                assert np.array_equal(occupied(want), occupied(e)) and np.array_equal(want[1][:, 5], e[1][:, 5])
            against_emulation(want, e, ma, mb, bins, f"{name} {H}x{W} bins {bins}")


@pytest.mark.parametrize("bins", (64, 512))
def test_default_grid_with_no_workgroup_to_give(lib, emu, bins):
    """One image more than the card has CUs: the default grid min(need, CUs / B) comes out at 0 and is raised to one workgroup per
    image.  On grid inputs with whole l, the rows where the two cosf part marked moving (as in test_device_grid_inputs_bit_for_bit),
    the cells, ratio and stats are those of blocks = 1 and the emulation's, bit for bit."""
    import ctypes
    B, H, W = int(torch.cuda.get_device_properties(0).multi_processor_count) + 1, 6, 10
    host = (ctypes.c_float * H)()
    emu._dll.pf_emu_odo_rows(H, host)
    agree = bits(np.array(host[:], np.float32)) == bits(oc.rows_of(lib, H, W, DEV))
    ma, mb, _ = oc.grid_maps(B, H, W, bins, 4.0, 13, integer=True)
    ma = (ma[0], ma[1], ma[2] | (~agree)[None, :, None].astype(np.uint8))
    got = oc.link_run(lib, ma, mb, DEV, bins=bins)
    print(f"[odometry] B = {B} (CUs + 1) bins {bins}: cos phi agrees on {int(agree.sum())} of {H} rows")
    assert agree.any() and got[2][:, 2 * bins + 1].all() and same(got, oc.link_run(lib, ma, mb, DEV, blocks=1, bins=bins))
    assert same(got, oc.link_run(emu, ma, mb, bins=bins))


def test_solve_reverse_and_track_beyond_a_wave_of_images(lib, emu):
    """pf_odo_solve, pf_odo_reverse_pose and pf_odo_track give a lane to an image, so image 64 is the first of a second workgroup:
    B = 65, a different scene per image on 6x10 maps.  The comparisons of test_device_link_matches_float64_and_the_emulation and of
    test_device_track_reverse_and_fuse_match_float64, and image b of the batch is image b run alone, bit for bit."""
    B, H, W = 65, 6, 10
    ma, mb = oc.many_maps(B, H, W, oc.lib_mapper(lib, DEV))
    for bins in (64, 512):
        got = oc.link_run(lib, ma, mb, DEV, bins=bins)
        oc.check_link(got, ma, mb, f"device B={B} {H}x{W} bins {bins}", bins=bins)
        for b in range(B):
            one = oc.link_run(lib, tuple(x[b:b + 1] for x in ma), tuple(x[b:b + 1] for x in mb), DEV, bins=bins)
            assert np.array_equal(one[2][0], got[2][b]) and np.array_equal(bits(one[0]), bits(got[0][b:b + 1])) \
                and np.array_equal(bits(one[1][0]), bits(got[1][b])), ("image alone", bins, b)
        against_emulation(got, oc.link_run(emu, ma, mb, bins=bins), ma, mb, bins, f"B={B} {H}x{W} bins {bins}")
    n = 6
    rng = np.random.default_rng(14)
    run, ref, alone = oc.TrackRun(lib, B, DEV), orf.Track(B), [oc.TrackRun(lib, 1, DEV) for _ in range(B)]
    for k in range(n):
        R = np.stack([er.axis_angle(rng.normal(size=3), rng.uniform(0, 40)) for _ in range(B)]).astype(np.float32)
        t = np.stack([pr.unit(rng.normal(size=3)) for _ in range(B)]).astype(np.float32)
        pv, lv = rng.random(B) < 0.8, rng.random(B) < 0.8
        ratio = np.exp2(rng.uniform(-1, 1, B)).astype(np.float32)
        t[~pv] = 0
        got = run.step(R, t, pv, ratio, lv)
        go, gc_, gs, gf = got
        ro, rc, rs, rf = ref.step(R, t, pv, ratio, lv)
        size = max(1.0, float(np.abs(rc).max()))
        assert np.array_equal(gf, rf), (k, gf, rf)
        assert np.abs(go - ro).max() <= 8 * er.U * (k + 1) and np.abs(gc_ - rc).max() <= 8 * er.U * (k + 1) * size, k
        assert (np.abs(gs / rs - 1) <= 8 * er.U * (k + 1)).all()
        Rr, tr = oc.reverse_run(lib, R, t, DEV)
        assert np.array_equal(bits(Rr), bits(np.ascontiguousarray(R.transpose(0, 2, 1)))) and np.abs(tr - orf.reverse_pose(R, t)[1]).max() <= 8 * er.U
        assert not np.signbit(tr[~pv]).any() and not tr[~pv].any()
        for b in range(B):
            one = alone[b].step(R[b:b + 1], t[b:b + 1], pv[b:b + 1], ratio[b:b + 1], lv[b:b + 1])
            assert all(np.array_equal(bits(o[0]), bits(g[b])) for o, g in zip(one, got)), ("video alone", k, b)
            R1, t1 = oc.reverse_run(lib, R[b:b + 1], t[b:b + 1], DEV)
            assert np.array_equal(bits(R1[0]), bits(Rr[b])) and np.array_equal(bits(t1[0]), bits(tr[b])), ("pose alone", k, b)
    state = run.state.cpu().numpy()
    assert all(np.array_equal(bits(alone[b].state.cpu().numpy()[0]), bits(state[b])) for b in range(B)), "the kept state"


def test_poisoned_state_and_reset_on_the_device(lib):
    from prior_flow_amd.odometry import Odometry
    H, W = 32, 64
    flows = oc.path_flows(H, W, oc.path_motions(W)[:3])
    fresh = oc.run_path(lib, flows, DEV)
    for junk, isum in ((float("nan"), 0x7FF8123456789ABC), (1e30, 2 ** 62), (-1e30, -2 ** 62)):
        odo = Odometry(1, H, W, DEV)
        oc.run_path(lib, flows[:2], DEV, odo=odo)
        for buf in (odo.state, odo.orientation, odo.centre, odo.baseline, odo.prev_baseline, odo.link_valid, odo.ratio, odo.link_stats,
                    odo.inv_depth, odo.depth_weight, odo.R_rev, odo.t_rev, odo.pose.R, odo.pose.t, odo.pose.stats) + odo.map_a[:3] + odo.map_b[:3]:
            buf.fill_(junk)
        for buf in (odo.flags, odo.disagree, odo.map_a[3], odo.map_b[3]):
            buf.fill_(77)
        odo.scale.hist.fill_(isum)
        odo.pose.sums.fill_(isum)
        odo.reset()
        got = oc.run_path(lib, flows, DEV, odo=odo)
        for g, f in zip(got, fresh):
            assert all(np.array_equal(bits(g[k]), bits(f[k])) for k in f if k != "pose"), junk
        assert not odo.scale.hist.any()


def test_device_track_reverse_and_fuse_match_float64(lib):
    B, n = 3, 12
    rng = np.random.default_rng(4)
    run, ref = oc.TrackRun(lib, B, DEV), orf.Track(B)
    for k in range(n):
        R = np.stack([er.axis_angle(rng.normal(size=3), rng.uniform(0, 40)) for _ in range(B)]).astype(np.float32)
        t = np.stack([pr.unit(rng.normal(size=3)) for _ in range(B)]).astype(np.float32)
        pv, lv = rng.random(B) < 0.8, rng.random(B) < 0.8
        ratio = np.exp2(rng.uniform(-1, 1, B)).astype(np.float32)
        t[~pv] = 0
        go, gc_, gs, gf = run.step(R, t, pv, ratio, lv)
        ro, rc, rs, rf = ref.step(R, t, pv, ratio, lv)
        size = max(1.0, float(np.abs(rc).max()))
        assert np.array_equal(gf, rf), (k, gf, rf)
        assert np.abs(go - ro).max() <= 8 * er.U * (k + 1) and np.abs(gc_ - rc).max() <= 8 * er.U * (k + 1) * size, k
        assert (np.abs(gs / rs - 1) <= 8 * er.U * (k + 1)).all()
        Rr, tr = oc.reverse_run(lib, R, t, DEV)
        assert np.array_equal(bits(Rr), bits(np.ascontiguousarray(R.transpose(0, 2, 1)))) and np.abs(tr - orf.reverse_pose(R, t)[1]).max() <= 8 * er.U
        assert not np.signbit(tr[~pv]).any() and not tr[~pv].any()
    H, W, B = 33, 70, 2
    a = th.some_maps(B, H, W)
    rng = np.random.default_rng(6)
    b = ((a[0] * np.exp2(rng.normal(0, 0.4, a[0].shape))).astype(np.float32), rng.random(a[1].shape).astype(np.float32), (rng.random(a[2].shape) < 0.1).astype(np.uint8))
    for S_a, S_b, lv in (((1.0, 0.5), (0.7, 2.0), (1, 1)), ((1.0, 1.0), (1.0, 1.0), (1, 0))):
        oc.check_fuse(oc.fuse_run(lib, a, b, S_a, S_b, lv, DEV), a, b, S_a, S_b, np.asarray(lv), f"device fuse lv={lv}")
    th.weightless(lib, a, b, DEV)


def test_python_layer_on_the_device():
    from prior_flow_amd._lib import PfError
    from prior_flow_amd.odometry import Odometry, ScaleLink, fuse_depth
    B, H, W = 1, 8, 16
    z = torch.zeros(B, 2, H, W, device=DEV)
    odo = Odometry(B, H, W, DEV)
    O, c = odo.push_flows(z, z)
    assert torch.equal(O.cpu(), torch.eye(3)[None]) and not bool(c.any()) and odo.flags.tolist() == [[1, 0, 0, 0]]
    m = (torch.zeros(B, H, W, device=DEV), torch.zeros(B, H, W, device=DEV), torch.zeros(B, H, W, dtype=torch.uint8, device=DEV))
    one = torch.ones(B, device=DEV)
    out = fuse_depth(m, m, one, one, one)
    assert [o.dtype for o in out] == [torch.float32, torch.float32, torch.uint8]
    for bad in (lambda: odo.push_flows(z.cpu(), z), lambda: odo.push_flows(z, z.cpu()), lambda: odo.push(z),
                lambda: ScaleLink(B, H, W, DEV).link(tuple(x.cpu() for x in m), m), lambda: fuse_depth(m, m, one.cpu(), one, one),
                lambda: fuse_depth(m, m, one, one, one, out=out[:2]), lambda: Odometry(B, H, W, "cpu"), lambda: ScaleLink(B, H, W, DEV, bins=48)):
        with pytest.raises(PfError):
            bad()


# ---- behind the bidirectional stream ---------------------------------------------------------------------------------------------
def by_hand(lib, r, st):
    """One push as its entry points called one by one on buffers of the caller; st: dict carried between pushes."""
    from prior_flow_amd import _lib
    from prior_flow_amd.odometry import _STATE0
    B, _, H, W = r.forward.shape
    f32 = lambda *s: torch.zeros(*s, device=DEV)                          # noqa: E731
    if not st:
        st.update(map_a=(f32(B, H, W), f32(B, H, W), torch.zeros(B, H, W, dtype=torch.uint8, device=DEV)),
                  state=torch.tensor(_STATE0, dtype=torch.float64, device=DEV).repeat(B, 1).contiguous(), baseline=torch.ones(B, device=DEV))
    steps = pc.stepwise(lib, r.forward.cpu().numpy(), r.occ_forward.cpu().numpy(), device=DEV)
    R, t, pstats = (torch.from_numpy(steps[-1][i]).to(DEV) for i in (2, 3, 4))
    kb, _, cb, mb = (torch.from_numpy(x).to(DEV) for x in pc.pmap(lib, r.forward.cpu().numpy(), steps[-1][2], steps[-1][3], r.occ_forward.cpu().numpy(), DEV))
    hist = torch.zeros(B, 2 * 512 + 2, dtype=torch.int64, device=DEV)
    ratio, lstats = f32(B), f32(B, 6)
    lib.odo_accumulate(st["map_a"], (kb, cb, mb), hist, 512, 4.0, 1e-4)
    lib.odo_solve(hist, ratio, lstats, H, W, 512, 4.0, 4, 0.05, 1.0)
    prev = st["baseline"].clone()
    orient, centre, flags = f32(B, 3, 3), f32(B, 3), torch.zeros(B, 4, dtype=torch.int32, device=DEV)
    lib.odo_track(R, t, pstats, ratio, lstats, st["state"], orient, centre, st["baseline"], flags)
    inv, wgt, dis = f32(B, H, W), f32(B, H, W), torch.zeros(B, H, W, dtype=torch.uint8, device=DEV)
    lib.odo_fuse(st["map_a"], (kb, cb, mb), prev, st["baseline"], lstats[:, 5].contiguous(), inv, wgt, dis, 0.05, 1e-4, 0.5)
    Rr, tr = f32(B, 3, 3), f32(B, 3)
    lib.odo_reverse_pose(R, t, Rr, tr)
    ka, _, ca, ma = (torch.from_numpy(x).to(DEV) for x in pc.pmap(lib, r.backward.cpu().numpy(), Rr.cpu().numpy(), tr.cpu().numpy(), r.occ_backward.cpu().numpy(), DEV))
    st["map_a"] = (ka, ca, ma)
    return dict(orientation=orient, centre=centre, baseline=st["baseline"].clone(), flags=flags, ratio=ratio, link_stats=lstats,
                inv_depth=inv, depth_weight=wgt, disagree=dis)


KEYS = ("orientation", "centre", "baseline", "flags", "ratio", "link_stats", "inv_depth", "depth_weight", "disagree")


def test_odometry_behind_the_stream_eager_and_captured():
    """A four-frame 128x256 sequence on the tiny model, iters = 2, occlusion "plane": Odometry.push equals the entry points called one
    by one bit for bit and allocates nothing after the first push; the push of the last pair, captured into ONE graph on an Odometry
    brought to the same state and replayed twice on copied-in inputs, gives the eager push's bits."""
    from prior_flow_amd.modules import state_dict_shapes
    from prior_flow_amd.odometry import Odometry
    from prior_flow_amd.prior_raft import PriOr_RAFT
    from prior_flow_amd.video import BidirectionalFlow, FlowStream
    B, H, W = 1, 128, 256
    m = PriOr_RAFT(argparse.Namespace(mixed_precision=False, dropout=0.0, alternate_corr=False))
    m.load_state_dict(gc.det_state_dict(state_dict_shapes()), strict=True)
    m = m.cuda().eval()
    f0, _ = gc.synthetic_pair(B, H, W, seed=5)
    frames = [torch.roll(f0, shifts=(t, 3 * t), dims=(2, 3)).cuda().contiguous() for t in range(4)]
    stream = FlowStream(m, iters=2, bidirectional=True, occlusion="plane")
    odo = Odometry(B, H, W, DEV)
    lib, st, results, want = odo.lib, {}, [], None
    with torch.no_grad():
        for frame in frames:
            r = stream(frame)
            if r is None:
                continue
            r = BidirectionalFlow(*[t.clone() if t is not None else None for t in r])
            torch.cuda.synchronize()
            n0 = torch.cuda.memory_stats()["allocation.all.allocated"]
            odo.push(r)
            if results:
                assert torch.cuda.memory_stats()["allocation.all.allocated"] == n0, "a push after the first allocated device memory"
            hand = by_hand(lib, r, st)
            for k in KEYS:
                assert torch.equal(getattr(odo, k), hand[k]), (len(results), k)
            assert not odo.scale.hist.any()
            results.append(r)
            want = {k: getattr(odo, k).clone() for k in KEYS}
    assert len(results) == 3
    print(f"[odometry] behind the stream: flags {odo.flags[0].tolist()}, link stats {odo.link_stats[0].tolist()}")
    cap = Odometry(B, H, W, DEV)
    for r in results[:2]:
        cap.push(r)
    saved = {k: v.clone() for k, v in dict(state=cap.state, baseline=cap.baseline, a0=cap.map_a[0], a2=cap.map_a[2], a3=cap.map_a[3]).items()}
    live = dict(state=cap.state, baseline=cap.baseline, a0=cap.map_a[0], a2=cap.map_a[2], a3=cap.map_a[3])
    last = results[2]
    src = BidirectionalFlow(*[torch.zeros_like(x) if x is not None else None for x in last])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        cap.push(src)                                                 # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap.push(src)
    for s, x in zip(src, last):
        if s is not None:
            s.copy_(x)
    for _ in range(2):
        for k, v in live.items():
            v.copy_(saved[k])                                         # the state before the third push
        for buf in (cap.orientation, cap.centre, cap.ratio, cap.link_stats, cap.inv_depth, cap.depth_weight):
            buf.fill_(float("nan"))
        cap.scale.hist.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for k in KEYS:
            assert torch.equal(getattr(cap, k), want[k]), k
        assert not cap.scale.hist.any()
