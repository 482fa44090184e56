"""Camera rotation from 360-degree flow on an MI355X: pf_ego_accumulate, pf_ego_solve, pf_ego_track,
pf_erp_rotate and pf_ego_derotate on the device against the float64 restatement (tests/egomotion_ref.py) under the bounds derived
there, and against the host emulation of the same header within those bounds (not bit for bit: the two sincosf differ);
reproducibility under repeated calls and other grids; poisoned buffers; the Python layer (prior_flow_amd.egomotion), eager and
captured, behind a bidirectional FlowStream.  Run with ``-m gpu``."""
import argparse

import numpy as np
import pytest
import torch

import egomotion_cases as ec
import egomotion_ref as er
import golden_cases as gc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def emu():
    return ec.emu()


@pytest.fixture(scope="module")
def lib():
    from prior_flow_amd._lib import load
    return load()


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def px(angle, W):
    return angle * W / (2 * np.pi)


@pytest.mark.parametrize("H,W", ec.SHAPES)
def test_device_estimates_match_float64_and_the_emulation(lib, emu, H, W):
    """Rest, the three rotations at B = 1..3, wound columns, masked junk and end points past a pole: the device holds the float64
    bounds, and lies within the same bound of the emulation."""
    worst = 0.0
    cases = [("rest", np.zeros((2, 2, H, W), np.float32), None, 4)]
    for B in (1, 2, 3):
        cases.append((f"rotations B={B}", ec.rotation_flows(B, H, W, rot=B)[0], None, 4))
    cases.append(("winding", ec.wound(ec.rotation_flows(3, H, W)[0], 7), None, 4))
    junk, bad = ec.poison(ec.rotation_flows(2, H, W, rot=1)[0], 5)
    cases.append(("masked", junk, bad, 4))
    cases.append(("junk without a mask", junk, None, 4))
    cases.append(("poles", ec.polar_flow(H, W, 11)[0], None, 1))
    for name, flow, mask, passes in cases:
        B = flow.shape[0]
        R, stats, sums = ec.estimate(lib, flow, mask, device="cuda", passes=passes)
        ref = er.Estimator(B, H, W, passes=passes).estimate(flow, mask)
        worst = max(worst, ec.check_rotation(R, stats, ref, f"device {name} {H}x{W}"))
        Re, se, _ = ec.estimate(emu, flow, mask, passes=passes)
        for b in range(B):
            assert er.angle_between(R[b], Re[b]) <= er.rotation_bound(ref[1][b, 3]), (name, b)
        assert same([stats[:, 2], stats[:, 4]], [se[:, 2], se[:, 4]]) and not sums.any(), name
    R, stats, sums = ec.estimate(lib, junk, np.ones_like(bad), np.stack([er.yaw(2, W)] * 2).astype(np.float32), device="cuda")
    assert same([R], [np.stack([er.yaw(2, W)] * 2).astype(np.float32)]) and not stats.any() and not sums.any()
    print(f"[egomotion] device {H}x{W}: worst angle / bound {worst:.4f}")


@pytest.mark.parametrize("H,W", ((32, 64), (48, 96)))
def test_device_robustness(lib, H, W):
    flow, truth = ec.robust_flow(H, W)
    first, _, _ = ec.estimate(lib, flow, device="cuda", passes=1)
    R, stats, _ = ec.estimate(lib, flow, device="cuda")
    a, b = px(er.angle_between(first[0], truth), W), px(er.angle_between(R[0], truth), W)
    print(f"[egomotion] device robust {H}x{W}: plain fit {a:.4f} px off, default estimate {b:.4f} px off")
    assert a > 1.0 and b < 0.05 and stats[0, 4] == 1


def test_same_bits_on_every_run_and_for_every_grid(lib):
    """Two runs, and grids of 1, 3 and 64 workgroups per image against the one chosen from the CU count: the raw sums of a plain and
    of a weighted pass, R and the stats are the same bits.  33x70 on one workgroup is 33 strips for 16 waves and 40x1100 nine
    strips to a row, the last one ragged: the strided loop and the tail of a row both run."""
    for (H, W), B in (((33, 70), 3), ((40, 1100), 2), ((6, 10), 1)):
        flow, _ = ec.rotation_flows(B, H, W)
        flow, bad = ec.poison(flow, 3)
        prev = np.stack([er.axis_angle((1, 0, 1), 2.0)] * B)
        want = None
        for blocks in (0, 0, 1, 3, 64):
            got = [ec.raw_sums(lib, flow, prev, False, bad, "cuda", blocks=blocks), ec.raw_sums(lib, flow, prev, True, bad, "cuda", blocks=blocks)]
            got += ec.estimate(lib, flow, bad, device="cuda", blocks=blocks)[:2]
            assert got[0].any() and got[1].any()
            want = got if want is None else want
            assert same(got, want), ((H, W), blocks)


def _one_image_more_than_cus():
    """(flow, mask, previous R) of CUs + 1 images on 6x10 maps, a different rotation per image, a tenth of the pixels junk."""
    B, H, W = int(torch.cuda.get_device_properties(0).multi_processor_count) + 1, 6, 10
    flow, bad = ec.poison(ec.many_rotation_flows(B, H, W, seed=23)[0], 3)
    return flow, bad, ec.small_rotations(B, 29)


def test_default_grid_with_no_workgroup_to_give(lib):
    """One image more than the card has CUs: the default grid min(need, CUs / B) comes out at 0 and is raised to one workgroup per
    image.  The raw sums of a plain and of a weighted pass are those of blocks = 1, bit for bit, and those of every 16th image
    (and the last) are the sums of that image run alone, where the default grid has workgroups to spare."""
    flow, bad, prev = _one_image_more_than_cus()
    B = flow.shape[0]
    for weighted in (False, True):
        got = ec.raw_sums(lib, flow, prev, weighted, bad, "cuda")
        assert got.any(1).all() and same([got], [ec.raw_sums(lib, flow, prev, weighted, bad, "cuda", blocks=1)]), weighted
        for b in sorted(set(range(0, B, 16)) | {B - 1}):
            one = ec.raw_sums(lib, flow[b:b + 1], prev[b:b + 1], weighted, bad[b:b + 1], "cuda")
            assert np.array_equal(one[0], got[b]), (weighted, "image alone", b)


def test_default_grid_sums_are_the_emulations(lib, emu):
    """The same launch against the emulation, bit for bit, on grid inputs (ec.grid_flows): every end point is a pixel centre, so
    both bearings come from cosf and sinf of the grid's own angles, and the pixels at whose angles the device's math library and the
    host's part are masked for both sides (as tests/test_hip_odometry.py does with its rows of cos phi).  Every other step of
    pf_ego_pixel is a correctly rounded fp32 operation on both sides.  On a scene with fractional end points the two libraries
    part at some angle of every image and no sum can be asked to agree: there the sums are held to
    blocks = 1 and to the image alone (the test above), here to all three."""
    B, H, W = int(torch.cuda.get_device_properties(0).multi_processor_count) + 1, 6, 10
    flow, c, r = ec.grid_flows(B, H, W, 31)
    agree, ok_r, ok_c = ec.grid_agreement(lib, H, W, c, r, "cuda")
    bad = (~agree | (np.random.default_rng(32).random((B, H, W)) < 0.1)).astype(np.uint8)
    prev = ec.small_rotations(B, 29)
    print(f"[egomotion] B = {B} (CUs + 1) grid inputs: cosf and sinf agree on {int(ok_r.sum())} of {H} rows and {int(ok_c.sum())} of {W} "
          f"columns, {(bad == 0).mean():.1%} of the pixels used")
    for weighted in (False, True):
        got = ec.raw_sums(lib, flow, prev, weighted, bad, "cuda")
        assert got[:, 11].all() and got[:, :9].any(1).all() and got[:, 10].all(), "an image without a used pixel or without a residual"
        assert same([got], [ec.raw_sums(lib, flow, prev, weighted, bad, "cuda", blocks=1)]), weighted
        want = ec.raw_sums(emu, flow, prev, weighted, bad)
        differ = got != want
        assert not differ.any(), (weighted, f"{int(differ.any(1).sum())} of {B} images, {int(differ.sum())} of {differ.size} cells differ",
                                  np.nonzero(differ.any(1))[0][:8].tolist())


def test_solve_and_track_beyond_a_wave_of_images(lib, emu):
    """pf_ego_solve and pf_ego_track give a lane to an image, so image 64 is the first of a second workgroup: B = 65 on 6x10 maps,
    a different rotation per image.  The estimate holds the float64 bounds and lies within them of the emulation's, the tracker
    holds its bound over twelve frames, and image b of the batch is image b run alone, bit for bit."""
    B, H, W = ec.MANY, 6, 10
    flow, _ = ec.many_rotation_flows(B, H, W)
    R, stats, sums = ec.estimate(lib, flow, device="cuda")
    ref = er.Estimator(B, H, W).estimate(flow)
    worst = ec.check_rotation(R, stats, ref, f"device B={B} {H}x{W}")
    Re, se, _ = ec.estimate(emu, flow)
    for b in range(B):
        assert er.angle_between(R[b], Re[b]) <= er.rotation_bound(ref[1][b, 3]), b
        Rb, sb, _ = ec.estimate(lib, flow[b:b + 1], device="cuda")
        assert same([Rb[0], sb[0]], [R[b], stats[b]]), ("image alone", b)
    assert same([stats[:, 2], stats[:, 4]], [se[:, 2], se[:, 4]]) and not sums.any() and stats[:, 4].all()
    T = 12
    Rs = np.stack([ec.small_rotations(T, 100 + b) for b in range(B)], 1)
    O, Cc, S = ec.track(lib, Rs, 0.9, "cuda")
    for b in range(B):
        tref = er.Tracker(0.9)
        for t in range(T):
            ro, rc = tref.push(Rs[t, b])
            assert np.abs(O[t, b] - ro).max() <= 2 * er.U and np.abs(Cc[t, b] - rc).max() <= 2 * er.U, (b, t)
        Ob, Cb, Sb = ec.track(lib, Rs[:, b], 0.9, "cuda")
        assert same([Ob, Cb], [O[:, b], Cc[:, b]]) and np.array_equal(Sb.view(np.uint64), S[:, b].view(np.uint64)), ("video alone", b)
    print(f"[egomotion] device B={B} {H}x{W}: worst angle / bound {worst:.4f}")


def test_poisoned_buffers_give_the_bits_of_a_fresh_estimator(lib):
    from prior_flow_amd.egomotion import RotationEstimator, Stabilizer
    B, H, W = 2, 33, 70
    flow, _ = ec.rotation_flows(B, H, W)
    tf = torch.from_numpy(flow).cuda()
    frame = torch.from_numpy(ec.smooth_frame(B, 3, H, W, 8)).cuda()
    fresh = Stabilizer(B, 3, H, W, "cuda", smoothing=0.5)
    want = [t.clone() for t in (fresh.push(frame, tf), fresh.estimator.R, fresh.estimator.stats, fresh.orientation, fresh.correction)]
    for junk, isum in ((float("nan"), 0x7FF8123456789ABC), (1e30, 2 ** 62), (-1e30, -2 ** 62)):
        st = Stabilizer(B, 3, H, W, "cuda", smoothing=0.5)
        e = st.estimator
        e.sums.fill_(isum)
        for t in (e.R, e.stats, st.orientation, st.correction, st.out):
            t.fill_(junk)
        got = [st.push(frame, tf), e.R, e.stats, st.orientation, st.correction]
        assert all(torch.equal(a, b) for a, b in zip(got, want)), junk
        assert not e.sums.any()


def test_device_tracking(lib):
    T = 300
    Rs = ec.small_rotations(T, 3)
    O, Cc, S = ec.track(lib, Rs, 0.9, "cuda")
    ref = er.Tracker(0.9)
    for t in range(T):
        ro, rc = ref.push(Rs[t])
        assert np.abs(O[t] - ro).max() <= 2 * er.U and np.abs(Cc[t] - rc).max() <= 2 * er.U, t
    assert (S[:, 0] >= 0).all() and (S[:, 4] >= 0).all()
    assert np.abs(O[-1].astype(np.float64).T @ O[-1] - np.eye(3)).max() <= 1e-6
    O1, C1, _ = ec.track(lib, Rs[:20], 1.0, "cuda")
    assert np.abs(C1 - O1).max() <= 2 * er.U
    _, C0, _ = ec.track(lib, Rs[:20], 0.0, "cuda")
    assert np.abs(C0 - np.eye(3)).max() <= 2 * er.U


@pytest.mark.parametrize("H,W", ((6, 10), (33, 70), (32, 64)))
def test_device_rotate_and_derotate(lib, emu, H, W):
    R = np.stack([er.axis_angle((1, 2, 3), 3.0), er.axis_angle((1, -1, 0.2), 120.0)]).astype(np.float32)
    for C in (1, 3, 4):
        frame = ec.smooth_frame(2, C, H, W, 20 + C)
        ec.check_rotated(ec.rotate(lib, frame, R, "cuda"), frame, R, er.rotate(frame, R), f"device rotate {H}x{W} C={C}")
        k = 3
        Rz = np.stack([er.yaw(k, W), er.yaw(-2 * k, W)])
        got = ec.rotate(lib, frame, Rz, "cuda")
        want = np.stack([np.roll(frame[0], -k, 2), np.roll(frame[1], 2 * k, 2)]).astype(np.float64)
        assert (np.abs(got - want) <= er.value_bound(frame, Rz, extra=3 * er.U)).all(), C
    if H > 6:
        fb = ec.smooth_frame(2, 3, H, W, 31, byte=True)
        ec.check_rotated_u8(ec.rotate(lib, fb, R, "cuda"), fb, R, er.rotate_u8(fb, R), f"device rotate bytes {H}x{W}")
    flow, truth = ec.rotation_flows(3, H, W)
    other = np.stack([er.yaw(0.6 * W, W), er.axis_angle((3, 1, 2), 170.0), er.axis_angle((0, 1, 0), 40.0)]).astype(np.float32)
    junk, bad = ec.poison(flow, 9)
    got, valid = ec.derotate(lib, junk, other, bad, "cuda")
    ec.check_derotated(got, valid, junk, other, er.derotate(junk, other, bad), f"device derotate {H}x{W}")
    ge, ve = ec.derotate(emu, junk, other, bad)
    assert np.array_equal(valid, ve)


def test_python_layer_on_the_device():
    from prior_flow_amd._lib import PfError
    from prior_flow_amd.egomotion import RotationEstimator, Stabilizer, derotate_flow, rotate_erp
    B, C, H, W = 1, 3, 8, 16
    f = torch.rand(B, C, H, W, device="cuda") * 255
    z = torch.zeros(B, 2, H, W, device="cuda")
    R = torch.eye(3, device="cuda").repeat(B, 1, 1)
    st = Stabilizer(B, C, H, W, "cuda")
    out = st.push(f, z)
    assert bool((st.estimator.stats[:, 4] == 1).all()) and torch.equal(out, rotate_erp(f, st.correction))
    assert er.angle_between(st.correction[0].cpu().numpy(), np.eye(3)) <= er.rotation_bound(4 / 3)
    # the identity removed from a zero flow: nothing, up to the chord bound in columns of the pole row (cos phi = sin(pi / 2 H))
    assert float(derotate_flow(z, R).abs().max()) <= er.CHORD * W / (2 * np.pi * np.sin(np.pi / (2 * H)))
    assert rotate_erp(f, R).shape == f.shape
    for bad in (lambda: st.push(f.cpu(), z), lambda: st.push(f, z.cpu()), lambda: st.push(f, z[:, :1]), lambda: st.push(f.double(), z),
                lambda: st.push(f, z, mask=torch.zeros(B, H, W, device="cuda")), lambda: st.push(f, z, out=f),
                lambda: derotate_flow(z.cpu(), R.cpu()), lambda: derotate_flow(z, R.cpu()), lambda: rotate_erp(f.cpu(), R.cpu()),
                lambda: rotate_erp(f[:, :, :, ::2], R), lambda: RotationEstimator(B, H, W, "cpu"), lambda: Stabilizer(B, C, H, W, "cpu"),
                lambda: Stabilizer(B, 5, H, W, "cuda"), lambda: RotationEstimator(B, H, W, "cuda", passes=0)):
        with pytest.raises(PfError):
            bad()


# ---- Stabilizer behind the bidirectional stream ---------------------------------------------------------------------------------
def test_stabilizer_behind_the_stream_eager_and_captured():
    """A four-frame 128x256 sequence on the tiny model of the splat test, iters = 2, occlusion "plane": push_bidirectional equals
    the pieces called one by one (estimate with the forward occlusion mask, pf_ego_track, rotate_erp) bit for bit; a push allocates
    nothing; the third push again, captured into ONE graph from a reset state and replayed twice on copied-in inputs, gives the
    eager call's bits.  The capture runs with torch's global error mode, under which a synchronisation inside the region raises."""
    from prior_flow_amd.egomotion import RotationEstimator, Stabilizer, rotate_erp
    from prior_flow_amd.modules import state_dict_shapes
    from prior_flow_amd.prior_raft import PriOr_RAFT
    from prior_flow_amd.video import BidirectionalFlow, FlowStream
    B, H, W = 1, 128, 256
    m = PriOr_RAFT(argparse.Namespace(mixed_precision=False, dropout=0.0, alternate_corr=False))
    m.load_state_dict(gc.det_state_dict(state_dict_shapes()), strict=True)
    m = m.cuda().eval()
    f0, _ = gc.synthetic_pair(B, H, W, seed=5)
    frames = [torch.roll(f0, shifts=(t, 3 * t), dims=(2, 3)).cuda().contiguous() for t in range(4)]
    stream = FlowStream(m, iters=2, bidirectional=True, occlusion="plane")
    st = Stabilizer(B, 3, H, W, "cuda", smoothing=0.8)
    est = RotationEstimator(B, H, W, "cuda")
    lib = st.lib
    state = st.state.clone()
    orient, corr = torch.zeros_like(st.orientation), torch.zeros_like(st.correction)
    results = []
    with torch.no_grad():
        for i, frame in enumerate(frames):
            r = stream(frame)
            if r is None:
                continue
            r = BidirectionalFlow(*[t.clone() if t is not None else None for t in r])
            torch.cuda.synchronize()
            n0 = torch.cuda.memory_stats()["allocation.all.allocated"]
            out = st.push_bidirectional(r, frame)
            assert torch.cuda.memory_stats()["allocation.all.allocated"] == n0, "a push allocated device memory"
            R = est.estimate(r.forward, r.occ_forward)
            lib.ego_track(R, state, orient, corr, 0.8)
            want = rotate_erp(frame, corr)
            assert torch.equal(R, st.estimator.R) and torch.equal(est.stats, st.estimator.stats)
            assert torch.equal(state, st.state) and torch.equal(orient, st.orientation) and torch.equal(corr, st.correction)
            assert torch.equal(out, want) and bool(torch.isfinite(out).all()) and not st.estimator.sums.any()
            results.append(r)
    assert len(results) == 3
    print(f"[egomotion] behind the stream: stats of the last pair {st.estimator.stats[0].tolist()}")
    # the third push alone from a reset state: eager, then captured and replayed twice on copied-in inputs
    eager = Stabilizer(B, 3, H, W, "cuda", smoothing=0.8)
    want = [t.clone() for t in (eager.push_bidirectional(results[2], frames[3]), eager.estimator.R, eager.correction, eager.state)]
    cap = Stabilizer(B, 3, H, W, "cuda", smoothing=0.8)
    src = BidirectionalFlow(*[torch.zeros_like(t) if t is not None else None for t in results[2]])
    a = torch.zeros_like(frames[3])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        cap.push_bidirectional(src, a)                            # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap.push_bidirectional(src, a)
    for s, t in zip(src, results[2]):
        if s is not None:
            s.copy_(t)
    a.copy_(frames[3])
    for _ in range(2):
        cap.reset()
        cap.out.fill_(float("nan"))
        cap.estimator.sums.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        got = (cap.out, cap.estimator.R, cap.correction, cap.state)
        assert all(torch.equal(x, y) for x, y in zip(got, want)) and not cap.estimator.sums.any()
