"""Depth along the trajectory on the device: pf_reproj_project within the float64 bound of
tests/reproject_ref.py; front, raw sums, outputs and hole bytes of the z-splat bit for bit the host emulation's (and the fp32
restatement's) on the same staged inputs; pf_depth_update bit for bit where no log2f decides; the truth of the analytic scenes; the
Python layer, its refusals, its state and a captured push behind a bidirectional FlowStream."""
import argparse

import numpy as np
import pytest
import torch

import golden_cases as gc
import reproject_cases as rc
import test_reproject_host as th

pytestmark = pytest.mark.gpu
bits = rc.bits
DEV = "cuda"


@pytest.fixture(scope="module")
def emu():
    return rc.emu()


@pytest.fixture(scope="module")
def lib():
    from prior_flow_amd._lib import load
    return load()


@pytest.mark.parametrize("B,H,W", ((1, 6, 10), (2, 17, 37), (3, 24, 48), (1, 33, 70), (2, 64, 128), (2, 40, 1100)))
def test_device_project_within_the_float64_bound(lib, B, H, W):
    d, w, mask, R, T = th.project_inputs(B, H, W, H)
    d[0, 0, :4] = [np.nan, np.inf, -1.0, 2.0 ** 30]
    w[0, 1, :3] = [0.0, -1.0, np.nan]
    got = rc.project_run(lib, d, w, R, T, mask, DEV)
    worst = th.check_project(got, d, w, mask, R, T, f"device {B}x{H}x{W}")
    print(f"[reproject] device project {B}x{H}x{W}: worst error / bound {worst:.3f}")
    again = rc.project_run(lib, d, w, R, T, mask, DEV)
    assert all((bits(a) == bits(b)).all() for a, b in zip(got, again)), "two runs, the same bits"
    Z = np.zeros((B, 3), np.float32)
    flow, dn, valid = rc.project_run(lib, d, w, R, Z, mask, DEV)
    assert (bits(dn[valid != 0]) == bits(d[valid != 0])).all(), "T = 0 changes no depth, bit for bit"
    flow, dn, valid = rc.project_run(lib, d, w, np.stack([np.eye(3, dtype=np.float32)] * B), Z, mask, DEV)
    assert (flow == 0).all() and (bits(dn[valid != 0]) == bits(d[valid != 0])).all(), "R = I, T = 0: nothing moves"


@pytest.mark.parametrize("B,C,H,W", rc.SWEEP)
def test_device_zsplat_bit_for_bit(lib, emu, B, C, H, W):
    """Every family of the sweep at one shape: the device against the emulation on the same staged inputs; twice; the element form."""
    for family in rc.FAMILIES:
        inp = rc.staged(family, B, C, H, W)
        run = rc.ZRun(lib, B, C, H, W, DEV)
        got = run.run(*inp)
        rc.same_bits(got, rc.zsplat_run(emu, *inp), f"device {family} {B}x{C}x{H}x{W}")
        assert not got[6].any() and not got[7].any(), "front and the sums are all-zero after a call"
        assert all(x is None or np.isfinite(x).all() for x in got[2:5]) and set(np.unique(got[5])) <= {0, 1}
        th.family_properties(family, inp, got)
        rc.same_bits(run.run(*inp), got, f"second run {family}")
        if family == "junk":
            rc.same_bits(got, rc.zsplat_run(lib, *rc.junk_as_invalid(*inp), device=DEV), "junk as invalid")
        if family in ("seam", "collapse"):
            rc.same_bits(rc.zsplat_run(lib, *inp, device=DEV, offset=1), got, f"unaligned maps {family}")


@pytest.mark.parametrize("B,H,W", ((1, 6, 10), (2, 17, 37), (3, 24, 48), (2, 40, 1100)))
def test_device_update(lib, emu, B, H, W):
    ds, ws, dm, wm, dis = rc.update_inputs(B, H, W, H)
    flags = np.array([[3, 2, 1, 1]] * B, np.int32)
    seg = np.full(B, 2, np.int32)
    seg[-1] = 1                                                             # the last image changes its segment
    got = rc.update_run(lib, ds, ws, dm, wm, dis, flags, seg, DEV)
    differ, worst, edge = th.check_update(got, ds, ws, dm, wm, dis, flags, seg, f"device update {B}x{H}x{W}")
    want = rc.update_run(emu, ds, ws, dm, wm, dis, flags, seg)
    apart = int((bits(got[0]) != bits(want[0])).sum() + (bits(got[1]) != bits(want[1])).sum())
    print(f"[reproject] device update {B}x{H}x{W}: worst error / bound {worst:.3f}; {differ} values differ from the fp32 restatement, "
          f"{apart} from the emulation, {edge} at the edge of tol")
    assert differ == 0 and apart == 0 and (got[2] == want[2]).all()
    unaligned = rc.update_run(lib, ds, ws, dm, wm, dis, flags, seg, DEV, offset=1)
    assert all((bits(a) == bits(b)).all() for a, b in zip(got, unaligned)), "the element form gives the quad form's bits"


def test_device_update_beyond_a_wave_of_images(lib, emu):
    """pf_depth_update's segment pass gives a lane to an image, so image 64 is the first of a second workgroup: B = 65 on 6x10
    maps, every second image (the last one too) changing its segment.  The comparisons of test_device_update, and image b of the
    batch is image b run alone, bit for bit."""
    B, H, W = 65, 6, 10
    ds, ws, dm, wm, dis = rc.update_inputs(B, H, W, 65)
    flags = np.array([[3, 2 + b % 3, 1, 1] for b in range(B)], np.int32)    # the segment each image is in now
    seg = np.where(np.arange(B) % 2 == 0, 1, flags[:, 1]).astype(np.int32)
    got = rc.update_run(lib, ds, ws, dm, wm, dis, flags, seg, DEV)
    differ, worst, edge = th.check_update(got, ds, ws, dm, wm, dis, flags, seg, f"device update {B}x{H}x{W}")
    want = rc.update_run(emu, ds, ws, dm, wm, dis, flags, seg)
    apart = int((bits(got[0]) != bits(want[0])).sum() + (bits(got[1]) != bits(want[1])).sum())
    print(f"[reproject] device update {B}x{H}x{W}: worst error / bound {worst:.3f}; {differ} values differ from the fp32 restatement, "
          f"{apart} from the emulation, {edge} at the edge of tol")
    assert differ == 0 and apart == 0 and (got[2] == want[2]).all() and (got[2] == flags[:, 1]).all()
    for b in range(B):
        one = rc.update_run(lib, *(x[b:b + 1] for x in (ds, ws, dm, wm, dis, flags, seg)), DEV)
        assert all((bits(o[0]) == bits(g[b])).all() for o, g in zip(one, got)), ("image alone", b)


def test_device_update_rules(lib):
    th.update_rules(lib, DEV)


def test_device_against_the_truth(lib):
    for H, W in rc.TRUTH_SHAPES:
        ref, got, d1, _ = th.truth_run(lib, rc.pair(rc.CONVEX, 0, H, W), DEV)
        e_ref, h_ref = rc.rel_error(ref[3][0], ref[5][0], d1)
        e_got, h_got = rc.rel_error(got[3][0], got[5][0], d1)
        print(f"[reproject] device convex {H}x{W}: worst relative error {e_got:.3e} (restatement {e_ref:.3e}), holes {h_got:.2%}")
        assert e_got <= 2 * e_ref and h_got <= rc.HOLE_CAP
    for H, W in rc.OCCLUDER_SHAPES:
        e_ref, e_got, e_bad = th.occluder_check(lib, H, W, DEV)
        assert e_got <= 1 and e_bad > 1


def test_device_filter_has_a_point(lib):
    H, W = 32, 64
    rf, rs = rc.filter_path(*rc.ref_filter(), H, W, 0)
    f, s = rc.filter_path(*rc.lib_filter(lib, DEV), H, W, 0)
    print(f"[reproject] device filter {H}x{W}: rms log2 error filtered / single = {f / s:.3f} (restatement {rf / rs:.3f})")
    assert f < s and f / s <= (rf / rs) * rc.FILTER_FACTOR


def test_python_layer_on_the_device():
    """Refusals launch nothing (acc, front still zero); poisoned state gives a fresh object's bits after reset()."""
    from prior_flow_amd._lib import PfError
    from prior_flow_amd.reproject import Reprojector, reproject, rigid_flow
    B, C, H, W = 2, 3, 24, 48
    d, w, mask, R, T = (torch.from_numpy(x).to(DEV) for x in th.project_inputs(B, H, W, 1))
    src = torch.rand(B, C, H, W, device=DEV) * 255
    rp = Reprojector(B, C, H, W, DEV)
    bad = [lambda: rp.run(src.cpu(), d, w, R, T), lambda: rp.run(src, d.cpu(), w, R, T), lambda: rp.run(src, d, w, R.cpu(), T),
           lambda: rp.run(src, d.double(), w, R, T), lambda: rp.run(src, d, w[:, :, :5], R, T), lambda: rp.run(None, d, w, R, T),
           lambda: rp.run(src, d.transpose(1, 2).contiguous().transpose(1, 2), w, R, T), lambda: rp.run(src, rp.inv_depth, w, R, T),
           lambda: rp.run(rp.out, d, w, R, T), lambda: rigid_flow(d.cpu(), w.cpu(), R.cpu(), T.cpu()),
           lambda: reproject(src, d, w, R, T, mask.float()), lambda: Reprojector(B, C, H, W, "cpu")]
    for i, f in enumerate(bad):
        with pytest.raises(PfError):
            f()
        assert not rp.acc.any() and not rp.front.any(), i
    want = [x.clone() for x in rp.run(src, d, w, R, T, mask)]
    once = reproject(src, d, w, R, T, mask)
    assert all(torch.equal(a, b) for a, b in zip(once, want))
    for x in (rp.flow, rp.d_new, rp.out, rp.inv_depth, rp.weight):
        x.fill_(float("nan"))
    rp.acc.fill_(1 << 40); rp.front.fill_(0x7F000000); rp.valid.fill_(255); rp.hole.fill_(255)
    rp.reset()
    assert all(torch.equal(a, b) for a, b in zip(rp.run(src, d, w, R, T, mask), want)), "reset() after poisoned state"
    rp.flow.fill_(1e30); rp.d_new.fill_(-1e30)
    rp.reset()
    assert all(torch.equal(a, b) for a, b in zip(rp.run(src, d, w, R, T, mask), want))


# ---- behind the bidirectional stream ---------------------------------------------------------------------------------------------
PROP_KEYS = ("inv_depth", "weight", "rigid_flow", "valid", "predicted_inv_depth", "predicted_weight", "hole", "predicted_frame", "seg")


def test_propagator_behind_the_stream_eager_and_captured():
    """A four-frame 128x256 sequence on the tiny model, iters = 2: DepthPropagator.push equals the entry points called one by one bit
    for bit and allocates nothing after the first push; the last push, captured into ONE graph after a side-stream warm-up and
    replayed twice from the state before it, gives the eager push's bits.  This exercises launches, state and capture, not the
    estimate, which is held to the truth on the analytic scenes."""
    from prior_flow_amd.modules import state_dict_shapes
    from prior_flow_amd.odometry import Odometry
    from prior_flow_amd.prior_raft import PriOr_RAFT
    from prior_flow_amd.reproject import DepthPropagator
    from prior_flow_amd.video import FlowStream
    B, H, W = 1, 128, 256
    m = PriOr_RAFT(argparse.Namespace(mixed_precision=False, dropout=0.0, alternate_corr=False))
    m.load_state_dict(gc.det_state_dict(state_dict_shapes()), strict=True)
    m = m.cuda().eval()
    f0, _ = gc.synthetic_pair(B, H, W, seed=5)
    frames = [torch.roll(f0, shifts=(t, 3 * t), dims=(2, 3)).cuda().contiguous() for t in range(4)]
    stream = FlowStream(m, iters=2, bidirectional=True, occlusion="plane")
    odo = Odometry(B, H, W, DEV)
    prop = DepthPropagator(odo, channels=3)
    lib = odo.lib
    ds, ws, seg = np.zeros((B, H, W), np.float32), np.zeros((B, H, W), np.float32), np.zeros(B, np.int32)
    pushes, prev, saved = 0, None, None
    with torch.no_grad():
        for frame in frames:
            r = stream(frame)
            if r is None:
                prev = frame
                continue
            odo.push(r)
            if pushes == 2:                                                # the state before the last push, for the replays
                saved = [x.clone() for x in (prop.rp.inv_depth, prop.rp.weight, prop.seg)]
            torch.cuda.synchronize()
            n0 = torch.cuda.memory_stats()["allocation.all.allocated"]
            prop.push(frame=prev)
            if pushes:
                assert torch.cuda.memory_stats()["allocation.all.allocated"] == n0, "a push after the first allocated device memory"
            # the same push, one entry point at a time on buffers of the test
            ud, uw, seg = rc.update_run(lib, ds, ws, odo.inv_depth.cpu().numpy(), odo.depth_weight.cpu().numpy(), odo.disagree.cpu().numpy(),
                                        odo.flags.cpu().numpy(), seg, DEV)
            assert np.array_equal(bits(prop.inv_depth.cpu().numpy()), bits(ud)) and np.array_equal(bits(prop.weight.cpu().numpy()), bits(uw))
            T = (odo.baseline[:, None] * odo.pose.t).cpu().numpy()
            flow, dn, valid = rc.project_run(lib, ud, uw, odo.pose.R.cpu().numpy(), T, odo.map_b[3].cpu().numpy(), DEV)
            z = rc.zsplat_run(lib, prev.cpu().numpy(), flow, dn, uw, valid, DEV)
            assert np.array_equal(bits(prop.rigid_flow.cpu().numpy()), bits(flow)) and np.array_equal(prop.valid.cpu().numpy(), valid)
            for a, b in zip((prop.predicted_frame, prop.predicted_inv_depth, prop.predicted_weight, prop.hole), z[2:6]):
                assert np.array_equal(bits(a.cpu().numpy()), bits(b)), pushes
            assert not prop.rp.acc.any() and not prop.rp.front.any()
            assert (seg == odo.flags[:, 1].cpu().numpy()).all()
            ds, ws = z[3], z[4]
            prev = frame
            pushes += 1
    assert pushes == 3
    print(f"[reproject] behind the stream: flags {odo.flags[0].tolist()}, state weight > 0 on {float((prop.weight > 0).float().mean()):.1%}, "
          f"holes {float(prop.hole.float().mean()):.1%}")
    want = {k: getattr(prop, k).clone() for k in PROP_KEYS}
    live = (prop.rp.inv_depth, prop.rp.weight, prop.seg)
    last = frames[2]                                                        # the earlier frame of the last pair
    src = torch.zeros_like(last)

    def restore():
        for x, s in zip(live, saved):
            x.copy_(s)
    restore()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        prop.push(frame=src)                                                # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(side)
    restore()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        prop.push(frame=src)
    src.copy_(last)
    for _ in range(2):
        restore()
        for buf in (prop.inv_depth, prop.weight, prop.rigid_flow, prop.predicted_frame):
            buf.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for k in PROP_KEYS:
            assert torch.equal(getattr(prop, k), want[k]), k
        assert not prop.rp.acc.any() and not prop.rp.front.any()
