"""Object tracks on the device: the vote matrix, track, age, origin, fate, next_id, track_map and the kept
state bit for bit the host emulation's on the device's own tables, step and path within twice the bound of tests/tracker_ref.py;
two runs, maps offset by one element and poisoned outputs give the same bits; the Python layer, its refusals and reset; an update +
push captured into a graph behind a bidirectional FlowStream; the moving ball over four frames."""
import argparse
from collections import namedtuple

import numpy as np
import pytest
import torch

import golden_cases as gc
import launch_paths as lp
import segments_cases as sc
import tracker_cases as tc

pytestmark = pytest.mark.gpu
DEV = "cuda"
R = namedtuple("R", "forward backward occ_forward occ_backward")


@pytest.fixture(scope="module")
def emu():
    return tc.emu()


@pytest.fixture(scope="module")
def lib():
    from prior_flow_amd._lib import load
    return load()


@pytest.mark.parametrize("B,H,W", tc.SHAPES)
def test_device_matches_the_emulation(lib, emu, B, H, W):
    rows, cols = sc.tables(lib, H, W, DEV)
    worst, runs = 0.0, 0
    for family in tc.FAMILIES:
        p = tc.pair(family, B, H, W)
        for M, min_area in tc.SETTINGS:
            o0, o1 = (tc.objects(lab, rows, cols, M, min_area) for lab in p["labels"])
            for direction in tc.DIRECTIONS:
                what = f"device {family} {B}x{H}x{W} M={M} {direction}"
                worst = max(worst, _device_against_emulation(lib, emu, p, o0, o1, rows, direction, M, what))
                runs += 1
    print(f"[tracker] device {B}x{H}x{W}: {runs} pairs, worst step / path difference / (2 x bound) {worst:.3f}")


def _device_against_emulation(lib, emu, p, o0, o1, rows, direction, M, what):
    """Two pushes on the device and in the emulation: every integer and the kept state bit for bit, step and path within twice the
    bound; a second run, maps offset by one element and poisoned outputs give the same bits.  -> worst difference / (2 x bound)."""
    worst = 0.0
    got = tc.run_pair(lib, p, o0, o1, rows, direction, M, DEV, ref=False)
    want = tc.run_pair(emu, p, o0, o1, rows, direction, M, ref=False)
    for k, (g, w) in enumerate(zip(got, want)):
        ints = tc.INT_KEYS + tc.STATE_KEYS[:-1]
        tc.same_bits({n: g[n] for n in ints}, {n: w[n] for n in ints}, f"{what} push {k + 1}")
        worst = max(worst, tc.within_bound(g, w, f"{what} push {k + 1}"))
        assert sc.bits(g["st_path"]).tolist() == sc.bits(g["path"]).tolist()
    for name, kw in (("second run", {}), ("maps offset by one element", dict(offset=1)), ("poisoned outputs", dict(poison=True))):
        again = tc.run_pair(lib, p, o0, o1, rows, direction, M, DEV, ref=False, **kw)
        for k in (0, 1):
            tc.same_bits(again[k], got[k], f"{name}: {what} push {k + 1}")
    return worst


def _cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.mark.parametrize("direction", tc.DIRECTIONS)
@pytest.mark.parametrize("family", tc.DEVICE_FAMILIES)
@pytest.mark.parametrize("case", tc.DEVICE_PATHS, ids=sc.case_id)
def test_device_matches_the_emulation_on_the_device_only_paths(lib, emu, case, family, direction):
    """The launch rules that no emulation restates: a vote grid capped by the CU count, whose workgroups go round their loop again
    (at twice the card's CUs in images a single workgroup of 16 waves takes 24 items, so half its waves find nothing the second
    time) and flush their LDS matrix or their global atomics after it; the table at PF_TRK_MAX_OBJECTS, where every thread of the
    match kernel owns a slot and the scan's last element is a real object."""
    cus = _cus()
    B, H, W = tc.device_case(case, cus)
    reached = set().union(*(lp.trk_device_paths(B, H, W, s[0], cus) for s in tc.DEVICE_SETTINGS))
    print(f"[tracker] device paths {lp.describe_trk(B, H, W, cus)}; reached: {sorted(reached)}")
    assert "table_256" in reached
    if case[0] == sc.TWO_PER_CU:
        assert lp.trk_vote_grid(B, H, W, cus) == (2, 1) and H * ((W + 63) // 64) == 24
    if case[0] == sc.TWO_PER_CU or cus < 512:
        assert {"vote_second_trip_lds", "vote_second_trip_global"} <= reached, f"{B}x{H}x{W} on {cus} CUs reaches {sorted(reached)}"
    small, full = tc.device_pair(family, B, H, W)
    rows, cols = sc.tables(lib, H, W, DEV)
    worst = 0.0
    for M, min_area in tc.DEVICE_SETTINGS:
        o0, o1 = (tc.objects(lab, rows, cols, M, min_area) for lab in small["labels"])
        if (case, family) == tc.OVERFLOWS and (M, min_area) == tc.FULL_TABLE:
            assert (o0[1] > M).all() and (o1[1] > M).all(), "the table of 256 is not full in both frames"
        what = f"device {family} {B}x{H}x{W} M={M} {direction}"
        worst = max(worst, _device_against_emulation(lib, emu, full, tc.tiled(o0, B), tc.tiled(o1, B), rows, direction, M, what))
    print(f"[tracker] device {B}x{H}x{W} {family} {direction}: worst step / path difference / (2 x bound) {worst:.3f}")


def _bits(tk):
    names = ("votes", "track", "age", "origin", "fate", "step", "path", "track_map", "next_id", "prev_ids", "prev_count", "prev_sums",
             "prev_track", "prev_age", "prev_path")
    return {n: getattr(tk, n).clone() for n in names}


def _equal(a, b):
    return all(torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)) for k in a)


def _poison(tk, state):
    names = ("votes", "track", "age", "origin", "fate", "step", "path", "track_map") \
        + (("next_id", "prev_ids", "prev_count", "prev_sums", "prev_track", "prev_age", "prev_path", "flow_prev", "flow_cur", "mask_prev",
            "mask_cur") if state else ())
    for n in names:
        x = getattr(tk, n)
        if x is not None:
            x.fill_(float("nan") if x.dtype.is_floating_point else (255 if x.dtype == torch.uint8 else -1))


def test_python_layer_on_the_device():
    """Refusals launch nothing (every buffer still zero, next_id still 1); a tracker whose outputs AND state were poisoned gives,
    after reset(), a fresh tracker's bits."""
    from prior_flow_amd._lib import PfError
    from prior_flow_amd.object_tracks import ObjectTracker
    from prior_flow_amd.segments import MovingObjects
    B, H, W = 2, 33, 70
    p = tc.pair("shift", B, H, W)
    dev = lambda a: torch.from_numpy(np.array(a)).to(DEV)                  # noqa: E731
    m0, m1, fw, bw = dev(p["masks"][0]), dev(p["masks"][1]), dev(p["fw"]), dev(p["bw"])
    occ = torch.zeros(B, H, W, dtype=torch.uint8, device=DEV)
    mo = MovingObjects(B, H, W, DEV, max_objects=8, min_area=0.0)
    tk = ObjectTracker(mo, grid="second")
    mo.update(m0)
    bad = [lambda: tk.link(None, None), lambda: tk.link(fw.cpu(), None), lambda: tk.link(fw, bw.cpu()), lambda: tk.link(fw, None, occ.cpu()),
           lambda: tk.link(fw.double(), None), lambda: tk.link(fw[:, :1].contiguous(), None), lambda: tk.link(fw, None, occ.int()),
           lambda: tk.link(fw, None, None, occ[:1]), lambda: tk.push(R(fw, None, None, None)), lambda: tk.push(R(fw.cpu(), bw, None, None)),
           lambda: tk.link(fw.transpose(2, 3).contiguous().transpose(2, 3), None), lambda: tk.push(fw),
           lambda: ObjectTracker(MovingObjects(B, H, W, DEV, max_objects=257)), lambda: ObjectTracker(mo, min_overlap=0.0),
           lambda: ObjectTracker(mo, min_overlap=float("nan")), lambda: ObjectTracker(mo, grid="both")]
    for i, f in enumerate(bad):
        with pytest.raises(PfError):
            f()
        assert not any(x.any() for k, x in _bits(tk).items() if k != "next_id") and (tk.next_id == 1).all(), i
    first_tk = ObjectTracker(mo, grid="first")
    with pytest.raises(PfError):
        first_tk.link(first_tk.flow_prev, None)                           # aliases the tracker's own buffer
    tk.push(R(fw, bw, occ, None))
    first = _bits(tk)
    mo.update(m1)
    track, age, track_map = tk.push(R(fw, bw, occ, None))
    want = _bits(tk)
    assert track[0, :2].tolist() == [1, 2] and age[:, :2].tolist() == [[2, 2]] * B and bool((track_map[mo.ids > 0] > 0).all())
    _poison(tk, state=True)
    tk.reset()
    mo.update(m0)
    tk.push(R(fw, bw, occ, None))
    assert _equal(_bits(tk), first), "a poisoned tracker after reset()"
    _poison(tk, state=False)
    mo.update(m1)
    tk.push(R(fw, bw, occ, None))
    assert _equal(_bits(tk), want), "poisoned outputs"


@pytest.mark.parametrize("H,W,theta", sc.BALL_SCENES)
def test_device_tracks_the_ball(emu, H, W, theta):
    seq = tc.ball_sequence(H, W, theta)
    tc.ball_track_check(tc.ball_track(seq, H, W, "cpu", emu), seq, f"emulation {H}x{W}")          # the restatement first
    tc.ball_track_check(tc.ball_track(seq, H, W, DEV), seq, f"device {H}x{W}")


def test_update_and_push_behind_the_stream_eager_and_captured():
    """Three frames at 128x256 on the tiny model, iters = 2, through a cold bidirectional FlowStream: a mask of each of its two
    pairs goes through MovingObjects.update + ObjectTracker.push, eagerly (allocating nothing) and as ONE captured graph that is
    replayed on copied-in inputs over poisoned outputs: the same bits after each pair."""
    from prior_flow_amd.modules import state_dict_shapes
    from prior_flow_amd.object_tracks import ObjectTracker
    from prior_flow_amd.prior_raft import PriOr_RAFT
    from prior_flow_amd.segments import MovingObjects
    from prior_flow_amd.video import FlowStream
    B, H, W = 1, 128, 256
    m = PriOr_RAFT(argparse.Namespace(mixed_precision=False, dropout=0.0, alternate_corr=False))
    m.load_state_dict(gc.det_state_dict(state_dict_shapes()), strict=True)
    m = m.cuda().eval()
    f0, _ = gc.synthetic_pair(B, H, W, seed=5)
    frames = [torch.roll(f0, shifts=(t, 3 * t), dims=(2, 3)).cuda().contiguous() for t in range(3)]
    stream = FlowStream(m, iters=2, bidirectional=True, occlusion="plane")
    u8 = lambda t: t.reshape(B, H, W).to(torch.uint8).contiguous().clone()  # noqa: E731
    with torch.no_grad():
        assert stream(frames[0]) is None
        pairs = []
        for f in frames[1:]:
            r = stream(f)
            pairs.append(R(r.forward.contiguous().clone(), r.backward.contiguous().clone(), u8(r.occ_forward), u8(r.occ_backward)))
        # the mask of each pair: its occluded pixels of the later frame and those whose backward u stands out (blobs that last)
        masks = [(p.occ_backward | ((p.backward[:, 0] - p.backward[:, 0].mean()).abs() > p.backward[:, 0].std()).to(torch.uint8)).contiguous()
                 for p in pairs]
        mo = MovingObjects(B, H, W, DEV, channels=2, min_area=0.5)
        tk = ObjectTracker(mo, grid="second")
        mo.update(masks[0], pairs[0].backward)
        tk.push(pairs[0])
        want = [_bits(tk)]
        torch.cuda.synchronize()
        n0 = torch.cuda.memory_stats()["allocation.all.allocated"]
        mo.update(masks[1], pairs[1].backward)
        tk.push(pairs[1])
        assert torch.cuda.memory_stats()["allocation.all.allocated"] == n0, "an update + push allocated device memory"
        want.append(_bits(tk))
        n = int(mo.count[0])
        print(f"[tracker] behind the stream: {n} objects in the second pair, {int((tk.age[0] > 1).sum())} of them continued, "
              f"next id {int(tk.next_id[0])}")
        # captured: static inputs, a warm-up on a side stream, one graph, then reset and replay per pair
        mo2 = MovingObjects(B, H, W, DEV, channels=2, min_area=0.5)
        tk2 = ObjectTracker(mo2, grid="second")
        static, mask = R(*(torch.zeros_like(t) for t in pairs[0])), torch.zeros_like(masks[0])
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            mo2.update(mask, static.backward)
            tk2.push(static)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            mo2.update(mask, static.backward)
            tk2.push(static)
        tk2.reset()
        for pair, mk, w in zip(pairs, masks, want):
            for dst, src in zip(static + (mask,), pair + (mk,)):
                dst.copy_(src)
            _poison(tk2, state=False)
            graph.replay()
            torch.cuda.synchronize()
            assert _equal(_bits(tk2), w)
