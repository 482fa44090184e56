"""Camera rotation from 360-degree flow without a GPU: the host emulation of pf_ego_accumulate,
pf_ego_solve, pf_ego_track, pf_erp_rotate and pf_ego_derotate (tests/emu/pf_emu_egomotion.cpp compiles csrc/pf_egomotion.h, the
header the device kernels compile) against the float64 restatement (tests/egomotion_ref.py) under the bounds derived there, exact
facts of the statement, the seeded faults, the scale rule, and the refusals of the Python layer.

Measured on the emulation (x86-64, glibc), worst error / bound: rotations 0.0014 (the bound is a worst case over every pixel; the
errors of the bearings average out), derotated flows 0.134, rotated fp32 frames 0.037; no rotated byte differs (0.40 % lie within
the bound of a half); tracking 9.5e-9 rad off the float64 product after 2 000 frames (bound 9.5e-4).  Robustness (pixel widths off
the truth, plain fit / default): 3.2006 / 0.0063 at 32x64, 3.2093 / 0.0063 at 48x96, the float64 statement and the emulation alike."""
import numpy as np
import pytest
import torch

import egomotion_cases as ec
import egomotion_ref as er


@pytest.fixture(scope="module")
def emu():
    return ec.emu()


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def px(angle, W):
    """An angle in pixel widths at the equator."""
    return angle * W / (2 * np.pi)


def robust_figures(first, default, truth, W):
    return px(er.angle_between(first, truth), W), px(er.angle_between(default, truth), W)


def check_robust(first, default, truth, W, what):
    a, b = robust_figures(first, default, truth, W)
    print(f"[egomotion] {what}: plain fit {a:.4f} px off, default estimate {b:.4f} px off")
    assert a > 1.0, (what, a)
    assert b < 0.05, (what, b)
    return a, b


# ---- exact facts ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", ec.SHAPES)
def test_rest(emu, H, W):
    """Zero flow: q == p bit for bit, so valid = 1, the gap is 4/3 up to the quadrature of the rows, every pixel is used and R is
    the identity within the bound."""
    flow = np.zeros((2, 2, H, W), np.float32)
    R, stats, sums = ec.estimate(emu, flow)
    ref = er.Estimator(2, H, W).estimate(flow)
    ec.check_rotation(R, stats, ref, f"rest {H}x{W}")
    for b in range(2):
        assert stats[b, 4] == 1 and stats[b, 2] == 1 and stats[b, 1] == 0
        assert abs(ref[1][b, 3] - 4 / 3) <= 1.0 / H ** 2 + 1e-9 and abs(stats[b, 3] - 4 / 3) <= 1.0 / H ** 2 + 64 * er.BEARING
        assert er.angle_between(R[b], np.eye(3)) <= er.rotation_bound(4 / 3)
    assert not sums.any()


@pytest.mark.parametrize("H,W", ec.SHAPES)
def test_pure_yaw(emu, H, W):
    """u = k, v = 0 is Rz(2 pi k / W) exactly."""
    for k in (1, 3, -2.5):
        flow = np.zeros((1, 2, H, W), np.float32)
        flow[:, 0] = k
        R, stats, _ = ec.estimate(emu, flow)
        err = er.angle_between(R[0], er.yaw(k, W))
        assert stats[0, 4] == 1 and err <= er.rotation_bound(stats[0, 3]), (k, err)


@pytest.mark.parametrize("H,W", ec.SHAPES)
def test_general_rotations(emu, H, W):
    """The three rotations of the sweep at B = 1..3, each image another one, against the statement and against the truth."""
    worst = 0.0
    for B in (1, 2, 3):
        flow, truth = ec.rotation_flows(B, H, W, rot=B)
        R, stats, sums = ec.estimate(emu, flow)
        ref = er.Estimator(B, H, W).estimate(flow)
        worst = max(worst, ec.check_rotation(R, stats, ref, f"rotations {H}x{W} B={B}"))
        for b in range(B):
            # the truth: the flow was rounded to fp32 (3 pi U on the sphere), which the bound's BEARING does not hold
            assert er.angle_between(R[b], truth[b]) <= er.rotation_bound(ref[1][b, 3]) * (1 + 3 * np.pi / 64), (B, b)
        assert not sums.any()
    print(f"[egomotion] {H}x{W}: worst angle / bound over the sweep {worst:.4f}")


@pytest.mark.parametrize("H,W", ec.SHAPES)
def test_winding(emu, H, W):
    """u +- W on a seeded half of the pixels: the same R within the bound."""
    flow, _ = ec.rotation_flows(3, H, W)
    R0, s0, _ = ec.estimate(emu, flow)
    R1, s1, _ = ec.estimate(emu, ec.wound(flow, 7))
    assert (ec.wound(flow, 7) != flow).mean() > 0.2
    for b in range(3):
        assert er.angle_between(R0[b], R1[b]) <= er.rotation_bound(s0[b, 3])
    ec.check_rotation(R1, s1, er.Estimator(3, H, W).estimate(flow), f"winding {H}x{W}")


@pytest.mark.parametrize("H,W", ((32, 64), (48, 96)))
def test_robustness(emu, H, W):
    """The experiment behind the defaults: the plain fit is dragged along by the moved block, the default estimate is not.  The
    float64 statement alone must meet the same two figures."""
    flow, truth = ec.robust_flow(H, W)
    ref = er.Estimator(1, H, W).estimate(flow, every_pass=True)
    check_robust(ref[0][0][0], ref[-1][0][0], truth, W, f"robust {H}x{W}, float64 statement")
    first, _, _ = ec.estimate(emu, flow, passes=1)
    R, stats, sums = ec.estimate(emu, flow)
    check_robust(first[0], R[0], truth, W, f"robust {H}x{W}, emulation")
    print(f"[egomotion] robust {H}x{W}: emulation against the statement {px(er.angle_between(R[0], ref[-1][0][0]), W):.2e} px")
    assert stats[0, 4] == 1 and not sums.any()


@pytest.mark.parametrize("H,W", ((33, 70), (32, 64)))
def test_end_points_past_a_pole_are_clamped(emu, H, W):
    flow, _ = ec.polar_flow(H, W, 11)
    R, stats, _ = ec.estimate(emu, flow, passes=1)
    ec.check_rotation(R, stats, er.Estimator(1, H, W, passes=1).estimate(flow), f"poles {H}x{W}")


@pytest.mark.parametrize("H,W", ec.SHAPES)
def test_masks_and_flows_that_are_not_finite(emu, H, W):
    """NaN, +-inf and 1e30 under the mask, and the same junk without a mask, give the bits of the call with those pixels masked
    and zero; with everything masked valid = 0, R = init and the sums are zero afterwards."""
    flow, _ = ec.rotation_flows(2, H, W, rot=1)
    junk, bad = ec.poison(flow, 5)
    clean = np.where(bad[:, None] != 0, np.float32(0), flow)
    want = ec.estimate(emu, clean, bad)
    for got in (ec.estimate(emu, junk, bad), ec.estimate(emu, junk, None)):
        assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1])) and not got[2].any()
    assert 0.8 < want[1][0, 2] < 0.97 and want[1][0, 4] == 1
    ec.check_rotation(want[0], want[1], er.Estimator(2, H, W).estimate(junk, bad), f"masked {H}x{W}")
    init = np.stack([er.axis_angle((0, 1, 1), 20.0), er.yaw(2, W)]).astype(np.float32)
    R, stats, sums = ec.estimate(emu, junk, np.ones_like(bad), init)
    assert np.array_equal(bits(R), bits(init)) and not stats.any() and not sums.any()


def test_the_order_of_the_adds_does_not_matter(emu):
    flow, _ = ec.rotation_flows(2, 33, 70)
    R = np.stack([er.axis_angle((1, 0, 1), 2.0)] * 2)
    try:
        got = []
        for seed in (0, 1, 12345):
            emu._dll.pf_emu_ego_order(seed)
            got.append(ec.raw_sums(emu, flow, R, True))
    finally:
        emu._dll.pf_emu_ego_order(0)
    assert got[0].any() and np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])


# ---- the scale rule ------------------------------------------------------------------------------------------------------------
def test_scale_rule(emu):
    """S = 62 - ceil(log2(H W)), S - 2 for the chord sum: at H W = 2^k and 2^k + 1 a sum whose every term is at its maximum stays
    at or below 2^62.  The worst case is run, not only computed: one row (cos phi = 1, so every weight is 1) at rest gives
    sum w = W 2^S exactly, and under the matrix -I every chord^2 is 4 |p|^2, so sum w r^2 reaches 4 W 2^(S-2) up to the rounding of
    |p|^2 and never passes it (the clamp)."""
    import ctypes
    out = (ctypes.c_int * 2)()
    for k in (1, 4, 12, 20, 29):
        for n in (2 ** k, 2 ** k + 1):
            emu._dll.pf_emu_ego_scales(1, n, out)
            S = 62 - int(np.ceil(np.log2(n)))
            assert (out[0], out[1]) == (S, S - 2) and n * 2 ** S <= 2 ** 62 and 4 * n * 2 ** (S - 2) <= 2 ** 62
            if k == 29:
                assert n * 2 ** (S + 1) > 2 ** 62              # one more bit would not fit: the scale is the largest safe one
    for W in (4096, 4097):
        flow = np.zeros((1, 2, 1, W), np.float32)
        S = 62 - int(np.ceil(np.log2(W)))
        s = ec.raw_sums(emu, flow, -np.eye(3)[None], False)[0]
        assert s[9] == W * 2 ** S and s[11] == W
        assert (1 - 8 * er.U) * W * 2 ** S <= int(s[10]) <= W * 2 ** S       # 4 |p|^2 with |p|^2 = 1 up to its fp32 roundings
        assert all(abs(int(v)) <= 2 ** 62 for v in s)
        # S_xx + S_yy = sum w (cos^2 + sin^2) up to the fp32 rounding of the squares
        assert abs(int(s[0]) + int(s[4]) - int(s[9])) <= 4 * er.U * int(s[9]) and s[8] == 0


# ---- tracking ------------------------------------------------------------------------------------------------------------------
def same_quat(got, want, t):
    """The state after step t against the statement's, sign included: a rounded matrix lies within 3 U of a rotation, and the two
    ways from it to a quaternion (the library's four-square rule, the statement's polar factor) part by no more than that, half of
    it in the quaternion, per step.  Where the scalar part is within the tolerance of zero either sign is the right one."""
    tol = 2 * er.U * (t + 1)
    err = np.abs(got - want).max()
    return err <= tol or (abs(want[0]) <= tol and np.abs(got + want).max() <= tol)


def test_tracking_over_2000_frames(emu):
    """2 000 seeded rotations: the orientation stays orthonormal to 1e-6 and within 8 T U of the float64 product of the same
    matrices (a rounded matrix lies within 3 U of its rotation, a product of T of them within 3 T U of the product of the
    rotations, its polar factor as near again; 2 U per step for the quaternion of a matrix that is not quite a rotation), and the
    state is the statement's quaternion, sign included."""
    T = 2000
    Rs = ec.small_rotations(T, 3)
    O, Cc, S = ec.track(emu, Rs, 1.0)
    P = np.eye(3)
    ref = er.Tracker(1.0)
    signs = 0
    for t in range(T):
        P = Rs[t].astype(np.float64) @ P
        ro, rc = ref.push(Rs[t])
        assert same_quat(S[t, :4], ref.o, t) and same_quat(S[t, 4:], ref.s, t), t
        signs += int(S[t, 0] < 1e-2)
    assert (S[:, 0] >= 0).all() and signs > 0                   # the scalar part came down to zero and stayed non-negative
    u, _, vt = np.linalg.svd(P)
    err = er.angle_between(O[-1], u @ vt)
    print(f"[egomotion] tracking: {err:.3e} rad from the float64 product after {T} frames, bound {8 * T * er.U:.3e}")
    assert err <= 8 * T * er.U
    for t in (0, T // 2, T - 1):
        assert np.abs(O[t].astype(np.float64).T @ O[t] - np.eye(3)).max() <= 1e-6
    assert np.abs(Cc - O).max() <= 2 * er.U                      # smoothing = 1: the correction is the orientation


def test_smoothing(emu):
    Rs = ec.small_rotations(60, 4)
    O, Cc, _ = ec.track(emu, Rs, 0.0)
    assert np.abs(Cc - np.eye(3)).max() <= 2 * er.U              # smoothing = 0: the video as it is
    O, Cc, S = ec.track(emu, Rs, 0.9)
    ref = er.Tracker(0.9)
    for t in range(60):
        ro, rc = ref.push(Rs[t])
        assert np.abs(O[t] - ro).max() <= 2 * er.U and np.abs(Cc[t] - rc).max() <= 2 * er.U, t
    assert er.angle_between(Cc[-1], np.eye(3)) > 0.05            # and it does correct something


# ---- the two appliers ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", ((6, 10), (33, 70), (32, 64)))
def test_rotate_fp32(emu, H, W):
    """Rz(2 pi k / W) is a roll by k columns; a general R is held to the statement; C = 1..4."""
    for C in (1, 3, 4):
        frame = ec.smooth_frame(2, C, H, W, 20 + C)
        k = 3
        Rz = np.stack([er.yaw(k, W), er.yaw(-2 * k, W)])
        got = ec.rotate(emu, frame, Rz)
        want = np.stack([np.roll(frame[0], -k, 2), np.roll(frame[1], 2 * k, 2)]).astype(np.float64)
        bound = er.value_bound(frame, Rz, extra=3 * er.U)
        assert (np.abs(got - want) <= bound).all(), (C, float((np.abs(got - want) / bound).max()))
        R = np.stack([er.axis_angle((1, 2, 3), 3.0), er.axis_angle((1, -1, 0.2), 120.0)]).astype(np.float32)
        ec.check_rotated(ec.rotate(emu, frame, R), frame, R, er.rotate(frame, R), f"rotate {H}x{W} C={C}")


@pytest.mark.parametrize("H,W", ((33, 70), (32, 64)))
def test_rotate_bytes(emu, H, W):
    frame = ec.smooth_frame(2, 3, H, W, 31, byte=True)
    R = np.stack([er.axis_angle((1, 2, 3), 3.0), er.axis_angle((1, -1, 0.2), 120.0)]).astype(np.float32)
    ref = er.rotate_u8(frame, R)
    bound = er.value_bound(frame.astype(np.float64).transpose(0, 3, 1, 2), R).transpose(0, 2, 3, 1)
    alone = float((np.abs(ref[0] + 0.5 - np.round(ref[0] + 0.5)) <= bound).mean())
    assert alone <= 0.02, alone                                  # the statement alone leaves room under the cap
    ec.check_rotated_u8(ec.rotate(emu, frame, R), frame, R, ref, f"rotate bytes {H}x{W}")
    k = 4
    Rz = np.stack([er.yaw(k, W)] * 2)
    assert np.array_equal(ec.rotate(emu, frame, Rz), np.roll(frame, -k, 2))


@pytest.mark.parametrize("H,W", ec.SHAPES)
def test_derotate(emu, H, W):
    """Derotating a rotation's own flow leaves nothing (on the sphere: u is unbounded at the poles); derotating by another
    rotation is held to the statement, wrapped u' included; left-out pixels give (0, 0) and clear valid."""
    flow, truth = ec.rotation_flows(3, H, W)
    R32 = truth.astype(np.float32)
    got, valid = ec.derotate(emu, flow, R32)
    m, n = er.grid(H, W)
    import viewport_ref as vr
    chord = np.linalg.norm(vr.sphere(m + got[:, 0].astype(np.float64), n + got[:, 1].astype(np.float64), H, W)
                           - vr.sphere(m, n, H, W)[None], axis=-1)
    assert valid.all() and chord.max() <= er.CHORD + 3 * er.U, chord.max()      # + the rounding of R_true to fp32
    other = np.stack([er.yaw(0.6 * W, W), er.axis_angle((3, 1, 2), 170.0), er.axis_angle((0, 1, 0), 40.0)]).astype(np.float32)
    junk, bad = ec.poison(flow, 9)
    got, valid = ec.derotate(emu, junk, other, bad)
    ec.check_derotated(got, valid, junk, other, er.derotate(junk, other, bad), f"derotate {H}x{W}")
    got2, valid2 = ec.derotate(emu, junk, other, None)
    assert np.array_equal(bits(got2), bits(got)) and np.array_equal(valid2, valid)


# ---- the seeded faults ---------------------------------------------------------------------------------------------------------
def _breaks(check):
    try:
        check()
    except AssertionError:
        return True
    return False


def test_seeded_faults_are_caught(emu):
    """Each mistake, built into a copy of the statement, must put at least one of the checks above outside its bound; without a
    fault the same checks pass."""
    H, W = 32, 64
    flow, truth = ec.rotation_flows(3, H, W)
    R, stats, _ = ec.estimate(emu, flow)
    pflow, _ = ec.polar_flow(H, W, 11)
    pR, pstats, _ = ec.estimate(emu, pflow, passes=1)
    rflow, rtruth = ec.robust_flow(H, W)
    Rs = ec.small_rotations(400, 3)
    _, _, S = ec.track(emu, Rs, 1.0)
    other = np.stack([er.yaw(0.6 * W, W), er.axis_angle((3, 1, 2), 170.0), er.axis_angle((0, 1, 0), 40.0)]).astype(np.float32)
    dgot, dvalid = ec.derotate(emu, flow, other)
    frame = ec.smooth_frame(3, 2, H, W, 2)
    fgot = ec.rotate(emu, frame, other)

    def checks(fault):
        def general():
            ec.check_rotation(R, stats, er.Estimator(3, H, W, fault=fault).estimate(flow), f"{fault}: rotations")

        def poles():
            ec.check_rotation(pR, pstats, er.Estimator(1, H, W, passes=1, fault=fault).estimate(pflow), f"{fault}: poles")

        def robust():
            ref = er.Estimator(1, H, W, fault=fault).estimate(rflow, every_pass=True)
            check_robust(ref[0][0][0], ref[-1][0][0], rtruth, W, f"{fault}: robust")

        def tracking():
            ref = er.Tracker(1.0, fault)
            for t in range(len(Rs)):
                ref.push(Rs[t])
                assert same_quat(S[t, :4], ref.o, t), t

        def derot():
            ec.check_derotated(dgot, dvalid, flow, other, er.derotate(flow, other, fault=fault), f"{fault}: derotate")

        def rot():
            ec.check_rotated(fgot, frame, other, er.rotate(frame, other, fault), f"{fault}: rotate")

        return {"general": general, "poles": poles, "robust": robust, "tracking": tracking, "derotate": derot, "rotate": rot}

    for name, check in checks(None).items():
        assert not _breaks(check), f"no fault: {name}"
    caught_by = {"r_transposed": ("general", "derotate", "rotate"), "no_cos_weight": ("general",), "row_not_clamped": ("poles",),
                 "no_reweight": ("robust",), "s_transposed": ("general",), "quat_sign": ("tracking",),
                 "sums_not_zeroed": ("general",), "u_not_wrapped": ("derotate",)}
    assert set(caught_by) == set(er.FAULTS)
    for fault, names in caught_by.items():
        c = checks(fault)
        for name in names:
            assert _breaks(c[name]), f"{fault} is not caught by {name}"


# ---- the Python layer ----------------------------------------------------------------------------------------------------------
def test_refusals(emu):
    from prior_flow_amd._lib import PfError
    from prior_flow_amd.egomotion import RotationEstimator, Stabilizer, derotate_flow, rotate_erp
    B, H, W = 2, 6, 10
    est = RotationEstimator(B, H, W, "cpu", lib=emu)
    flow = torch.zeros(B, 2, H, W)
    R = torch.eye(3).repeat(B, 1, 1)
    frame = torch.zeros(B, 3, H, W)
    stab = Stabilizer(B, 3, H, W, "cpu", lib=emu)
    stab8 = Stabilizer(B, 4, H, W, "cpu", form="u8", lib=emu)
    assert stab8.push(torch.zeros(B, H, W, 4, dtype=torch.uint8), flow).shape == (B, H, W, 4)
    before = est.R.clone()
    for bad in (lambda: est.estimate(flow.double()), lambda: est.estimate(flow[:1]), lambda: est.estimate(flow[:, :, :, ::2]),
                lambda: est.estimate(flow.transpose(2, 3).contiguous().transpose(2, 3)),
                lambda: est.estimate(flow, mask=torch.zeros(B, H, W)), lambda: est.estimate(flow, mask=torch.zeros(B, H, 1, dtype=torch.uint8)),
                lambda: est.estimate(flow, init=R.double()), lambda: est.estimate(flow, init=est.R), lambda: est.estimate(flow.numpy()),
                lambda: RotationEstimator(B, H, W, "cpu"), lambda: RotationEstimator(B, H, W, "cpu", passes=0, lib=emu),
                lambda: RotationEstimator(B, H, W, "cpu", passes=1.5, lib=emu), lambda: RotationEstimator(B, H, W, "cpu", scale_px=0.0, lib=emu),
                lambda: RotationEstimator(B, 0, W, "cpu", lib=emu), lambda: RotationEstimator(B, 1 << 15, 1 << 15, "cpu", lib=emu),
                lambda: derotate_flow(flow, R), lambda: derotate_flow(flow, R[:1], lib=emu), lambda: derotate_flow(flow, R.double(), lib=emu),
                lambda: derotate_flow(flow, R, valid=torch.zeros(B, H, W), lib=emu), lambda: derotate_flow(flow[:, :1], R, lib=emu),
                lambda: rotate_erp(frame, R), lambda: rotate_erp(frame, R, out=frame, lib=emu), lambda: rotate_erp(frame.double(), R, lib=emu),
                lambda: rotate_erp(torch.zeros(B, 5, H, W), R, lib=emu), lambda: rotate_erp(torch.zeros(B, 0, H, W), R, lib=emu),
                lambda: rotate_erp(torch.zeros(B, H, W, 5, dtype=torch.uint8), R, lib=emu),
                lambda: rotate_erp(frame, R, out=torch.zeros(B, 3, H, W, dtype=torch.uint8), lib=emu),
                lambda: rotate_erp(frame[:, :, :, ::2], R, lib=emu),
                lambda: Stabilizer(B, 5, H, W, "cpu", lib=emu), lambda: Stabilizer(B, 3, H, W, "cpu", form="f16", lib=emu),
                lambda: Stabilizer(B, 3, H, W, "cpu", smoothing=1.5, lib=emu), lambda: Stabilizer(B, 3, H, W, "cpu", passes=0, lib=emu),
                lambda: stab.push(frame.to(torch.uint8), flow), lambda: stab.push(frame, flow, out=frame),
                lambda: stab.push(frame[:, :2], flow), lambda: stab.push_bidirectional((flow, flow), frame)):
        with pytest.raises(PfError):
            bad()
    assert torch.equal(est.R, before) and not est.sums.any()     # a refused call has launched nothing
    # the C entries answer before anything is launched
    d = emu._dll
    keep = [torch.zeros(64) for _ in range(5)]
    p = [t.data_ptr() for t in keep]
    assert d.pf_ego_accumulate(None, None, p[1], p[2], 1, 4, 4, 0, 1.0, 0, None) == -1
    assert d.pf_ego_accumulate(p[0], None, p[1], p[2], 1, 4, 4, 2, 1.0, 0, None) == -1
    assert d.pf_ego_accumulate(p[0], None, p[1], p[2], 1, 4, 4, 0, 0.0, 0, None) == -1
    assert d.pf_ego_accumulate(p[0], None, p[1], p[2], 1, 4, 4, 0, 1.0, 65536, None) == -1
    assert d.pf_ego_accumulate(p[0], None, p[1], p[2], 0, 4, 4, 0, 1.0, 0, None) == -2
    assert d.pf_ego_accumulate(p[0], None, p[1], p[2], 1, 1 << 15, 1 << 15, 0, 1.0, 0, None) == -2
    assert d.pf_ego_solve(p[2], None, p[1], p[1], 1, 4, 4, 1e-3, None) == -1
    assert d.pf_ego_solve(p[2], None, p[1], p[3], 1, 4, 4, -1.0, None) == -1
    assert d.pf_ego_track(p[1], p[2], p[3], p[3], 1, 1.0, None) == -1
    assert d.pf_ego_track(p[1], p[2], p[3], p[4], 1, 1.5, None) == -1
    assert d.pf_erp_rotate(p[0], p[0], p[1], 1, 3, 4, 4, 0, None) == -1
    assert d.pf_erp_rotate(p[0], p[2], p[1], 1, 5, 4, 4, 0, None) == -1
    assert d.pf_erp_rotate(p[0], p[2], p[1], 1, 3, 4, 4, 2, None) == -1
    assert d.pf_ego_derotate(p[0], None, p[1], None, None, 1, 4, 4, None) == -1
    assert d.pf_ego_scratch_bytes(3, 4, 4) == 3 * 96 and d.pf_ego_scratch_bytes(3, 0, 4) == -2
