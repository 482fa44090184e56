"""Camera translation from 360-degree flow without a GPU: the host emulation of pf_epi_accumulate,
pf_epi_solve and pf_epi_map (tests/emu/pf_emu_epipolar.cpp compiles csrc/pf_epipolar.h, the header the device kernels compile)
against the float64 restatement (tests/epipolar_ref.py) under the bounds derived there, launch by launch; the restatement itself
against the truth of the seeded scenes; degenerate and junk inputs; order and state; the seeded faults; the refusals.

Figures of the restatement and of the emulation are in DESIGN.md section 20 (clean scenes, robust scene, worst error / bound)."""
import ctypes

import numpy as np
import pytest
import torch

import egomotion_ref as er
import epipolar_cases as pc
import epipolar_ref as pr


@pytest.fixture(scope="module")
def emu():
    return pc.emu()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same_bits(a, b, keys=("R", "t", "stats", "R0", "sums", "ego_sums")):
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in keys)


# ---- against float64 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,B,depth", [(H, W, B, d) for (H, W) in pc.SHAPES for B, d in ((1, "smooth"), (2, "room"), (3, "smooth"))]
                         + [(40, 1100, 1, "smooth")])
def test_against_float64(emu, H, W, B, depth):
    """Every launch of the default schedule, and the map of its answer, within the bounds; PoseEstimator is those launches."""
    flow, _, _, _ = pc.scene(B, H, W, depth)
    mask = (np.random.default_rng(5).random((B, H, W)) < 0.1).astype(np.uint8) if B == 2 else None
    steps = pc.stepwise(emu, flow, mask)
    pc.check_steps(steps, flow, mask, what=f"emulation {depth} {H}x{W} B={B}")
    got = pc.estimate(emu, flow, mask)
    assert np.array_equal(bits(got["R"]), bits(steps[-1][2])) and np.array_equal(bits(got["t"]), bits(steps[-1][3]))
    assert np.array_equal(bits(got["stats"]), bits(steps[-1][4])) and np.array_equal(bits(got["R0"]), bits(steps[0][2]))
    assert not got["sums"].any() and not got["ego_sums"].any()
    pc.check_map(pc.pmap(emu, flow, got["R"], got["t"], mask), flow, got["R"], got["t"], pr.parallax(flow, got["R"], got["t"], mask),
                 f"emulation map {depth} {H}x{W} B={B}")


# ---- against the truth -----------------------------------------------------------------------------------------------------------
def truth_figures(R, t, R0, R_true, t_true, W):
    return pr.px(pr.angle_vec(t, t_true), W), pr.px(er.angle_between(R, R_true), W), pr.px(er.angle_between(R0, R_true), W)


@pytest.mark.parametrize("H,W", ((32, 64), (48, 96)))
@pytest.mark.parametrize("depth", ("smooth", "room"))
def test_clean_scenes_against_the_truth(emu, H, W, depth):
    """The restatement, and the emulation, on every (rotation, translation, baseline) of the lists: t within 0.5 pixel widths, the
    refined R no worse than the rotation-only fit, and kappa = |T| / rho wherever conf >= 0.05, within the triangulation's
    sensitivity to the pose error that was measured on the restatement: 4 (dt + dR) (1 + kappa) / |q x t|."""
    worst = [0.0, 0.0, 0.0]
    for rot in range(3):
        flow, R_true, t_true, kap = pc.scene(3, H, W, depth, rot=rot, tr=0, base=rot)
        ref = pr.Pose(3, H, W).estimate(flow)
        got = pc.estimate(emu, flow)
        for name, (R, t, R0) in (("restatement", (ref[0], ref[1], ref[3])), ("emulation", (got["R"], got["t"], got["R0"]))):
            k, _, conf, moving, _ = pr.parallax(flow, R, t) if name == "restatement" else pc.pmap(emu, flow, R, t) + (None,)
            for b in range(3):
                et, eR, eR0 = truth_figures(R[b], t[b], R0[b], R_true[b], t_true[b], W)
                worst = [max(worst[0], et), max(worst[1], eR), max(worst[2], eR / eR0)]
                assert et <= 0.5, (name, rot, b, "t", et)
                assert eR <= eR0, (name, rot, b, "the R pass made R worse", eR, eR0)
                on = conf[b] >= 0.05
                turn = (et + eR) * 2 * np.pi / W + 4 * pr.NORMAL
                tol = 4 * turn * (1 + kap[b]) / np.sqrt(np.maximum(conf[b], 0.05))
                assert (np.abs(k[b] - kap[b])[on] <= tol[on]).all(), (name, rot, b, "kappa", np.abs(k[b] - kap[b])[on].max())
                assert not moving[b].any(), (name, rot, b, "a static scene has moving pixels", int(moving[b].sum()))
    print(f"[epipolar] clean {depth} {H}x{W}: worst t {worst[0]:.5f} px, R {worst[1]:.5f} px, R / rotation-only {worst[2]:.4f}")


@pytest.mark.parametrize("H,W", ((32, 64), (48, 96)))
@pytest.mark.parametrize("vote_px", (0.1, 0.25, 0.5))
def test_robust_scene(emu, H, W, vote_px):
    """A block of 7.5 % of the pixels moved by (6, -2) px: t within 0.5 px, recall of the block >= 0.9, false alarms <= 0.002 of
    the static pixels; the float64 statement alone must meet the same figures."""
    flow, R_true, t_true, blk = pc.robust_scene(H, W)
    ref = pr.Pose(1, H, W, vote_px=vote_px).estimate(flow)
    got = pc.estimate(emu, flow, vote_px=vote_px)
    for name, R, t, mov in (("restatement", ref[0], ref[1], pr.parallax(flow, ref[0], ref[1])[3]),
                            ("emulation", got["R"], got["t"], pc.pmap(emu, flow, got["R"], got["t"])[3])):
        et, eR = pr.px(pr.angle_vec(t[0], t_true), W), pr.px(er.angle_between(R[0], R_true), W)
        recall, false = float(mov[0][blk].mean()), float(mov[0][~blk].mean())
        print(f"[epipolar] robust {H}x{W} vote_px {vote_px} {name}: t {et:.4f} px, R {eR:.4f} px, recall {recall:.3f}, false {false:.5f}")
        assert et <= 0.5 and recall >= 0.9 and false <= 0.002, (name, et, recall, false)
    pc.check_steps(pc.stepwise(emu, flow, vote_px=vote_px), flow, what=f"emulation robust {H}x{W} vote_px {vote_px}", vote_px=vote_px)


def test_translation_at_a_pole(emu):
    H, W = 32, 64
    rho = pr.depth_smooth(H, W)
    R_true = er.axis_angle((1, 2, 3), 3.0)
    for sign in (1.0, -1.0):
        flow = pr.scene_flow(R_true, (0, 0, sign), 0.3, rho)[None].astype(np.float32)
        ref = pr.Pose(1, H, W).estimate(flow)
        steps = pc.stepwise(emu, flow)
        pc.check_steps(steps, flow, what=f"emulation t at pole {sign:+.0f}")
        for t in (ref[1][0], steps[-1][3][0]):
            assert pr.px(pr.angle_vec(t, (0, 0, sign)), W) <= 0.5


# ---- degenerate and junk inputs ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("rotation", "rest"))
def test_no_epipole(emu, kind):
    """A pure rotation, and rest: valid = 0, t = t_init or zero, R = the rotation estimate bit for bit, a map of zeros."""
    B, H, W = 2, 32, 64
    flow = pc.ec.rotation_flows(B, H, W)[0] if kind == "rotation" else np.zeros((B, 2, H, W), np.float32)
    t_init = np.array([[0.6, 0, 0.8], [0, 1, 0]], np.float32)
    for init in (None, t_init):
        got = pc.estimate(emu, flow, init_t=init)
        assert not got["stats"][:, 5].any(), got["stats"]
        assert np.array_equal(got["t"], np.zeros((B, 3), np.float32) if init is None else init)
        assert np.array_equal(bits(got["R"]), bits(got["R0"]))
        k, r, c, m = pc.pmap(emu, flow, got["R"], np.zeros((B, 3)))
        assert not k.any() and not r.any() and not c.any() and not m.any()
        ref = pr.Pose(B, H, W).estimate(flow, init_t=init)
        assert not ref[2][:, 5].any()


def test_everything_masked(emu):
    B, H, W = 2, 33, 70
    flow, R, t, _ = pc.scene(B, H, W)
    mask = np.ones((B, H, W), np.uint8)
    for mode in (0, 1):
        assert not pc.raw_sums(emu, flow, R, t, mode, mask).any()
    got = pc.estimate(emu, flow, mask)
    assert not got["stats"].any() and not got["t"].any()
    k, r, c, m = pc.pmap(emu, flow, R, t, mask)
    assert not k.any() and not r.any() and not c.any() and not m.any()


def test_junk_flows_are_left_out(emu):
    """NaN, +-inf and +-1e30 on a seeded tenth of the pixels give the BITS of the same call with those pixels masked and zeroed."""
    B, H, W = 2, 33, 70
    flow, R, t, _ = pc.scene(B, H, W)
    junk, bad = pc.ec.poison(flow, 3)
    clean = np.where(bad[:, None] != 0, np.float32(0), flow)
    assert same_bits(pc.estimate(emu, junk), pc.estimate(emu, clean, bad))
    for mode in (0, 1):
        assert np.array_equal(pc.raw_sums(emu, junk, R, t, mode), pc.raw_sums(emu, clean, R, t, mode, bad))
    a, b = pc.pmap(emu, junk, R, t), pc.pmap(emu, clean, R, t, bad)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def test_wound_columns_and_thrown_end_points(emu):
    """u +- W on a seeded half of the pixels: the restatement is periodic, the code is held to it.  A twentieth of the end points
    thrown past a pole: the row clamp."""
    H, W = 33, 70
    flow, _, _, _ = pc.scene(2, H, W, "room")
    wound = pc.wound_half(flow, 11)
    pc.check_steps(pc.stepwise(emu, wound), wound, what="emulation wound")
    assert np.array_equal(pr.Pose(2, H, W).estimate(wound)[2][:, 5], pr.Pose(2, H, W).estimate(flow)[2][:, 5])
    pflow, _, _ = pc.polar_scene(H, W, 12)
    steps = pc.stepwise(emu, pflow)
    pc.check_steps(steps, pflow, what="emulation poles")
    pc.check_map(pc.pmap(emu, pflow, steps[-1][2], steps[-1][3]), pflow, steps[-1][2], steps[-1][3],
                 pr.parallax(pflow, steps[-1][2], steps[-1][3]), "emulation poles map")


# ---- order and state -------------------------------------------------------------------------------------------------------------
def test_add_order_does_not_matter(emu):
    B, H, W = 2, 33, 70
    flow, R, t, _ = pc.scene(B, H, W)
    try:
        want = [pc.raw_sums(emu, flow, R, t, mode) for mode in (0, 1)]
        for order in (1, 7, 12345):
            emu._dll.pf_emu_epi_order(order)
            for mode in (0, 1):
                assert np.array_equal(pc.raw_sums(emu, flow, R, t, mode), want[mode]), (order, mode)
    finally:
        emu._dll.pf_emu_epi_order(0)
    # a pass adds only to the sums its solve reads
    assert not want[0][:, 13:].any() and not want[1][:, :9].any() and not want[1][:, 10:12].any()
    assert want[0][:, :13].all() and want[1][:, 13:].all() and (want[0][:, 12] == H * W).all() and (want[1][:, 12] == H * W).all()


@pytest.mark.parametrize("W", (4096, 4097))
def test_worst_case_row_does_not_overflow(emu, W):
    """Every pixel at the maximum: n 2^S (and n 4 2^(S-2)) stays at or below 2^62, at a power of two and one past it."""
    out = (ctypes.c_longlong * 2)()
    emu._dll.pf_emu_epi_worst(1, W, out)
    lg = int(np.ceil(np.log2(W)))
    assert out[0] == out[1] == W << (62 - lg) and 0 < out[0] <= 1 << 62


def test_poisoned_buffers(emu):
    """Buffers full of NaN / +-1e30, and the sums with the same bit patterns, give the bits of a fresh PoseEstimator."""
    B, H, W = 2, 33, 70
    flow, _, _, _ = pc.scene(B, H, W)
    fresh = pc.estimate(emu, flow)
    for junk in (float("nan"), 1e30, -1e30):
        est = pc.estimator(emu, B, H, W)
        for buf in (est.R, est.t, est.stats, est.estimator.R, est.estimator.stats):
            buf.fill_(junk)
        pat = int(np.array([junk], np.float32).view(np.int32)[0])
        est.sums.fill_(pat * (1 << 32) + pat)
        est.estimator.sums.fill_(pat * (1 << 32) + pat)
        assert same_bits(pc.estimate(emu, flow, est=est), fresh), junk
        assert same_bits(pc.estimate(emu, flow, est=est), fresh), junk     # and again on its own leftovers


# ---- the seeded faults -------------------------------------------------------------------------------------------------------------
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
    flow, _, _, _ = pc.scene(3, H, W)
    steps = pc.stepwise(emu, flow)
    R, t = steps[-1][2], steps[-1][3]
    kmap = pc.pmap(emu, flow, R, t)
    rflow, _, rt_true, blk = pc.robust_scene(H, W)
    rsteps = pc.stepwise(emu, rflow)
    pflow, _, _ = pc.polar_scene(H, W, 12)
    psteps = pc.stepwise(emu, pflow)

    def checks(fault):
        def general():
            pc.check_steps(steps, flow, what=f"{fault}: clean", fault=fault)

        def robust():
            pc.check_steps(rsteps, rflow, what=f"{fault}: robust", fault=fault)

        def truth():
            ref = pr.Pose(1, H, W, fault=fault).estimate(rflow)
            mov = pr.parallax(rflow, ref[0], ref[1])[3]
            assert pr.px(pr.angle_vec(ref[1][0], rt_true), W) <= 0.5 and mov[0][blk].mean() >= 0.9 and mov[0][~blk].mean() <= 0.002

        def poles():
            pc.check_steps(psteps, pflow, what=f"{fault}: poles", fault=fault)

        def pmap():
            pc.check_map(kmap, flow, R, t, pr.parallax(flow, R, t, fault=fault), f"{fault}: map")

        return {"general": general, "robust": robust, "truth": truth, "poles": poles, "map": pmap}

    for name, check in checks(None).items():
        assert not _breaks(check), f"no fault: {name}"
    caught_by = {"no_cos_weight": ("general",), "no_vote_norm": ("truth",), "no_reweight": ("robust",), "no_sign": ("general",),
                 "r_transposed": ("general", "map"), "dw_right": ("general",), "kappa_swapped": ("map",),
                 "row_not_clamped": ("poles",), "sums_not_zeroed": ("general",)}
    assert set(caught_by) == set(pr.FAULTS)
    for fault, names in caught_by.items():
        c = checks(fault)
        for name in names:
            assert _breaks(c[name]), f"{fault} is not caught by {name}"


# ---- the Python layer and the argument checks ----------------------------------------------------------------------------------------
def test_refusals(emu):
    from prior_flow_amd._lib import PfError
    from prior_flow_amd.parallax import PoseEstimator, parallax_map
    B, H, W = 2, 6, 10
    est = PoseEstimator(B, H, W, "cpu", lib=emu)
    flow = torch.zeros(B, 2, H, W)
    R = torch.eye(3).repeat(B, 1, 1)
    t = torch.zeros(B, 3)
    before = est.R.clone()
    for bad in (lambda: est.estimate(flow.double()), lambda: est.estimate(flow[:1]), lambda: est.estimate(flow[:, :, :, ::2]),
                lambda: est.estimate(flow, mask=torch.zeros(B, H, W)), lambda: est.estimate(flow, init_t=t.double()),
                lambda: est.estimate(flow, init_t=est.t), lambda: est.estimate(flow, init_t=torch.zeros(B, 4)),
                lambda: est.estimate(flow, init_R=est.estimator.R), lambda: est.estimate(flow.numpy()),
                lambda: est.estimate_bidirectional((flow, flow)),
                lambda: PoseEstimator(B, H, W, "cpu"), lambda: PoseEstimator(B, H, W, "cpu", t_passes=0, lib=emu),
                lambda: PoseEstimator(B, H, W, "cpu", rounds=1.5, lib=emu), lambda: PoseEstimator(B, H, W, "cpu", vote_px=0.0, lib=emu),
                lambda: PoseEstimator(B, H, W, "cpu", scale_px=-1.0, lib=emu), lambda: PoseEstimator(B, H, W, "cpu", passes=0, lib=emu),
                lambda: PoseEstimator(B, 0, W, "cpu", lib=emu), lambda: PoseEstimator(B, 1 << 15, 1 << 15, "cpu", lib=emu),
                lambda: parallax_map(flow, R, t), lambda: parallax_map(flow, R[:1], t, lib=emu), lambda: parallax_map(flow, R, t.double(), lib=emu),
                lambda: parallax_map(flow[:, :1], R, t, lib=emu), lambda: parallax_map(flow, R, t, mask=torch.zeros(B, H, W), lib=emu),
                lambda: parallax_map(flow, R, t, out=(t, t, t), lib=emu), lambda: parallax_map(flow, R, t, thr_px=-1.0, lib=emu),
                lambda: parallax_map(flow, R, t, out=tuple(torch.zeros(B, H, W) for _ in range(4)), lib=emu)):
        with pytest.raises(PfError):
            bad()
    assert torch.equal(est.R, before) and not est.sums.any()     # a refused call has launched nothing
    assert len(parallax_map(flow, R, t, lib=emu)) == 4


def test_argument_checks(emu):
    """Each rule of the *_check functions once; every one answers before anything is launched.  -1 = PF_ERR_BAD_ARG, -2 =
    PF_ERR_BAD_SHAPE."""
    d = emu._dll
    keep = [torch.zeros(64) for _ in range(9)]
    f, R, t, s, st, o1, o2, o3, ti = [x.data_ptr() for x in keep]
    acc = lambda flow=f, mask=None, R=R, t=t, sums=s, B=1, H=4, W=4, mode=0, sc=1.0, vp=0.25, blocks=0: d.pf_epi_accumulate(  # noqa: E731
        flow, mask, R, t, sums, B, H, W, mode, sc, vp, blocks, None)
    assert acc() == 0 and acc(t=None) == 0 and acc(mode=1) == 0
    for kw in (dict(flow=None), dict(R=None), dict(sums=None), dict(sums=s + 4), dict(sums=f), dict(R=s), dict(t=s), dict(t=R),
               dict(mode=2), dict(mode=-1), dict(mode=1, t=None), dict(blocks=-1), dict(blocks=65536), dict(sc=0.0), dict(sc=float("inf")),
               dict(sc=float("nan")), dict(vp=0.0), dict(vp=-1.0), dict(vp=1e-30)):
        assert acc(**kw) == -1, kw
    for kw in (dict(B=0), dict(H=0), dict(W=0), dict(B=65536), dict(H=1 << 15, W=1 << 15)):
        assert acc(**kw) == -2, kw
    sol = lambda sums=s, ti=None, R=R, t=t, st=st, B=1, H=4, W=4, mode=0, gap=1e-3, par=0.05: d.pf_epi_solve(  # noqa: E731
        sums, ti, R, t, st, B, H, W, mode, gap, par, None)
    keep[3].zero_()
    assert sol() == 0 and sol(R=None) == 0 and sol(ti=ti) == 0
    for kw in (dict(sums=None), dict(t=None), dict(st=None), dict(sums=s + 4), dict(t=s), dict(st=s), dict(R=s), dict(t=st), dict(ti=t),
               dict(ti=st), dict(R=t), dict(R=st), dict(R=ti, ti=ti), dict(mode=2), dict(mode=1, R=None), dict(gap=-1.0),
               dict(gap=float("nan")), dict(par=-1.0), dict(par=float("inf"))):
        assert sol(**kw) == -1, kw
    for kw in (dict(B=0), dict(H=0), dict(H=1 << 15, W=1 << 15)):
        assert sol(**kw) == -2, kw
    mp = lambda flow=f, mask=None, R=R, t=t, k=o1, r=o2, c=o3, m=None, B=1, H=4, W=4, thr=1.0, neg=0.5, cm=0.05: d.pf_epi_map(  # noqa: E731
        flow, mask, R, t, k, r, c, m, B, H, W, thr, neg, cm, None)
    assert mp() == 0 and mp(k=None, r=None, c=None) == 0
    for kw in (dict(flow=None), dict(R=None), dict(t=None), dict(t=R), dict(k=f), dict(r=R), dict(c=t), dict(m=f), dict(k=o2),
               dict(c=o1), dict(mask=o1), dict(thr=-1.0), dict(neg=float("nan")), dict(cm=-0.1), dict(cm=float("inf"))):
        assert mp(**kw) == -1, kw
    for kw in (dict(B=0), dict(W=0), dict(H=1 << 15, W=1 << 15)):
        assert mp(**kw) == -2, kw
    assert d.pf_epi_sums_bytes(3, 4, 4) == 3 * 22 * 8 and d.pf_epi_sums_bytes(3, 0, 4) == -2
