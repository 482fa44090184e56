"""Connected components on the cyclic panorama, on the device: labels, ids, keep, roots, count and every
64-bit sum bit for bit the host emulation's on the device's own tables, the table within the float64 bound of
tests/segments_ref.py; two runs, unaligned maps and poisoned buffers give the same bits; the Python layer, its refusals, a captured
update behind a bidirectional FlowStream; the analytic moving-ball scene."""
import argparse

import numpy as np
import pytest
import torch

import golden_cases as gc
import launch_paths as lp
import segments_cases as sc
import segments_ref as sr

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def emu():
    return sc.emu()


@pytest.fixture(scope="module")
def lib():
    from prior_flow_amd._lib import load
    return load()


def _table_within_bound(got, what):
    """The device's table against the float64 evaluation of the device's own sums (which are the emulation's, bit for bit)."""
    B, M, F = got["table"].shape
    H, W = got["labels"].shape[1:]
    want, bound = np.zeros((B, M, F)), np.zeros((B, M, F))
    for b in range(B):
        for k in range(min(int(got["count"][b]), M)):
            want[b, k], bound[b, k] = sr.resolve(got["sums"][b, k], F - sr.COLS, H, W)
    assert np.isfinite(got["table"]).all(), what
    worst = sr.table_error(got["table"], want, bound, W)
    assert worst <= 1.0, f"{what}: table error / bound = {worst:.3f}"
    return worst


def _device_against_emulation(lib, emu, m, v, setting, tabs, what):
    """One update on the device and in the emulation: every integer bit for bit, the table within the bound, and a second run,
    maps offset by one element and poisoned buffers give the same bits.  -> (worst table error / bound, the device's arrays)."""
    conn, poles, M, min_area = setting
    W = m.shape[2]
    got = sc.run(lib, m, v, conn, poles, M, min_area, DEV, tabs=tabs)
    want = sc.run(emu, m, v, conn, poles, M, min_area, tabs=tabs)
    for k in ("labels", "ids", "keep", "roots", "count", "sums"):
        bad = sc.bits(got[k]) != sc.bits(want[k])
        assert not bad.any(), f"{what}: {k} differs in {int(bad.sum())} of {bad.size} cells, first at {np.argwhere(bad)[0].tolist()}"
    worst = max(_table_within_bound(got, what), sr.table_error(got["table"], want["table"].astype(np.float64), _bound_of(got), W))
    sc.same_bits(sc.run(lib, m, v, conn, poles, M, min_area, DEV, tabs=tabs), got, f"second run: {what}")
    sc.same_bits(sc.run(lib, m, v, conn, poles, M, min_area, DEV, offset=1, tabs=tabs), got, f"unaligned maps: {what}")
    sc.same_bits(sc.run(lib, m, v, conn, poles, M, min_area, DEV, tabs=tabs, poison=True), got, f"poisoned buffers: {what}")
    return worst, got


@pytest.mark.parametrize("B,C,H,W", sc.SWEEP)
def test_device_matches_the_emulation(lib, emu, B, C, H, W):
    tabs = sc.tables(lib, H, W, DEV)
    v = sc.values(B, C, H, W)
    worst, runs = 0.0, 0
    for family in sc.FAMILIES:
        m = sc.mask(family, B, H, W)
        for setting in sc.combos(family):
            what = f"device {family} {B}x{C}x{H}x{W} {setting}"
            worst = max(worst, _device_against_emulation(lib, emu, m, v, setting, tabs, what)[0])
            runs += 1
    print(f"[segments] device {B}x{C}x{H}x{W}: {runs} cases, worst table error / bound {worst:.3f}")


def _cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


# what each of sc.DEVICE_PATHS is there for (tests/launch_paths.py); the second trip of the product size hangs on the card's CUs
REACHES = {
    (sc.TWO_PER_CU, 1, 24, 48): {"accumulate_second_trip_lds", "accumulate_second_trip_global"},
    (2, 3, 512, 1024): {"scan_two_rows_per_thread"},
    (1, 1, 257, 66): {"scan_two_rows_per_thread", "scan_clipped_threads"},
    (1, 0, 600, 8): {"scan_two_rows_per_thread", "scan_clipped_threads"},
}


@pytest.mark.parametrize("family", sc.DEVICE_FAMILIES)
@pytest.mark.parametrize("case", sc.DEVICE_PATHS, ids=sc.case_id)
def test_device_matches_the_emulation_on_the_device_only_paths(lib, emu, case, family):
    """The launch rules that no emulation restates: an accumulate grid capped by the CU count, whose workgroups go round their loop
    again and flush their LDS partials (or their global atomics) once after it; a scan in which a thread holds two or three rows
    and the last threads are clipped; the tables at 512 (the largest kept in LDS) and at PF_SEG_MAX_OBJECTS, both full."""
    cus = _cus()
    B, C, H, W = sc.device_case(case, cus)
    reached = set().union(*(lp.seg_device_paths(B, C, H, W, s[2], cus) for s in sc.device_combos(family)))
    print(f"[segments] device paths {lp.describe_seg(B, C, H, W, cus)}; reached: {sorted(reached)}")
    assert REACHES[case] <= reached, f"{B}x{C}x{H}x{W} on {cus} CUs reaches {sorted(reached)}"
    if case == sc.OVERFLOWS[0]:
        assert cus >= 512 or {"accumulate_second_trip_lds", "accumulate_second_trip_global"} <= reached
    assert {"table_512", "table_4096"} <= reached
    if case == (1, 1, 257, 66):
        assert lp.seg_scan_rows_per_thread(H) == 2 and lp.seg_scan_rows_of_thread(H, 128) == 1 and lp.clipped_threads(H)[1] == 129
    if case == (1, 0, 600, 8):
        assert lp.seg_scan_rows_per_thread(H) == 3 and lp.clipped_threads(H)[0] == 200 and lp.seg_scan_rows_of_thread(H, 200) == 0
    tabs = sc.tables(lib, H, W, DEV)
    m, v = sc.mask(family, B, H, W), sc.values(B, C, H, W)
    worst = 0.0
    for setting in sc.device_combos(family):
        what = f"device {family} {B}x{C}x{H}x{W} {setting}"
        w, got = _device_against_emulation(lib, emu, m, v, setting, tabs, what)
        worst = max(worst, w)
        if (case, family) == sc.OVERFLOWS and setting in sc.FULL_TABLES:
            assert (got["count"] > setting[2]).all() and (got["roots"] >= 0).all(), f"{what}: the table is not full"
    print(f"[segments] device {B}x{C}x{H}x{W} {family}: {len(sc.device_combos(family))} settings, worst table error / bound {worst:.3f}")


def _bound_of(got):
    """Twice the reference's bound: the device and the emulation may each be off by one of them."""
    B, M, F = got["table"].shape
    H, W = got["labels"].shape[1:]
    bound = np.zeros((B, M, F))
    for b in range(B):
        for k in range(min(int(got["count"][b]), M)):
            bound[b, k] = 2 * sr.resolve(got["sums"][b, k], F - sr.COLS, H, W)[1]
    return bound


def test_device_tables(lib, emu):
    """The tables are cos and sin of the row and column angles to fp32 accuracy (4 ulp of a value up to 1)."""
    for H, W in ((1, 1), (33, 70), (130, 257)):
        rows, cols = sc.tables(lib, H, W, DEV)
        ph = (0.5 - (np.arange(H) + 0.5) / H) * np.pi
        th = ((np.arange(W) + 0.5) / W - 0.5) * 2 * np.pi
        tol = 4 * sr.U + 8 * sr.U * np.pi                        # the function, and its argument rounded in fp32
        assert np.abs(rows - np.stack([np.cos(ph), np.sin(ph)], 1)).max() <= tol and (rows[:, 0] >= 0).all()
        assert np.abs(cols - np.stack([np.cos(th), np.sin(th)], 1)).max() <= tol


def _state(mo):
    return {k: getattr(mo, k).clone() for k in ("labels", "ids", "keep", "roots", "count", "table", "sums")}


def _equal(a, b):
    return all(torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)) for k in a)


def test_python_layer_on_the_device():
    """Refusals launch nothing (every buffer still zero); an object whose buffers were poisoned gives a fresh object's bits."""
    from prior_flow_amd._lib import PfError
    from prior_flow_amd.segments import MovingObjects, label_components
    B, C, H, W = 2, 3, 33, 70
    m = torch.from_numpy(sc.mask("bernoulli_0.5", B, H, W).copy()).to(DEV)
    v = torch.from_numpy(sc.values(B, C, H, W).copy()).to(DEV)
    mo = MovingObjects(B, H, W, DEV, channels=C, poles=True)
    bad = [lambda: mo.update(m.cpu(), v), lambda: mo.update(m, v.cpu()), lambda: mo.update(m, None), lambda: mo.update(m.float(), v),
           lambda: mo.update(m[:, :, :5], v), lambda: mo.update(m, v.double()), lambda: mo.update(m, v[:, :2].contiguous()),
           lambda: mo.update(m.transpose(1, 2).contiguous().transpose(1, 2), v), lambda: mo.update(mo.keep, v),
           lambda: mo.update_parallax(m, v[:, :2].contiguous(), v[:, :2].contiguous(), v[:, 0].cpu()),
           lambda: label_components(m.cpu()), lambda: label_components(m, connectivity=6), lambda: MovingObjects(B, H, W, "cpu"),
           lambda: MovingObjects(B, H, W, DEV, max_objects=4097), lambda: MovingObjects(B, H, W, DEV, min_area=-1.0)]
    for i, f in enumerate(bad):
        with pytest.raises(PfError):
            f()
        assert not any(x.any() for x in (mo.labels, mo.ids, mo.keep, mo.roots, mo.count, mo.sums, mo.table)), i
    mo.update(m, v)
    want = _state(mo)
    assert int(want["count"].sum()) > 0 and torch.equal(label_components(m, poles=True), want["labels"])
    for x in (mo.labels, mo.ids, mo.roots, mo.count, mo.sums, mo._t.scratch):
        x.fill_(-1)
    mo.keep.fill_(255)
    mo.table.fill_(float("nan"))
    mo.update(m, v)
    assert _equal(_state(mo), want), "poisoned buffers"
    fresh = MovingObjects(B, H, W, DEV, channels=C, poles=True)
    fresh.update(m, v)
    assert _equal(_state(fresh), want), "a fresh object"


@pytest.mark.parametrize("H,W,theta", sc.BALL_SCENES)
def test_device_finds_the_ball(lib, emu, H, W, theta):
    from prior_flow_amd.segments import MovingObjects
    s = sc.ball_scene(H, W, theta)
    host = MovingObjects(1, H, W, "cpu", channels=3, lib=emu)
    _, hcount, htable = host.update_parallax(*(torch.from_numpy(s[k]) for k in ("moving", "flow", "rigid_flow", "inv_depth")))
    sc.ball_check(htable.numpy(), hcount.numpy(), s, W, f"emulation {H}x{W}")            # the restatement first
    mo = MovingObjects(1, H, W, DEV, channels=3)
    ids, count, table = mo.update_parallax(*(torch.from_numpy(s[k]).to(DEV) for k in ("moving", "flow", "rigid_flow", "inv_depth")))
    sc.ball_check(table.cpu().numpy(), count.cpu().numpy(), s, W, f"device {H}x{W}")
    assert int(mo.keep.sum()) < int(s["moving"].sum()), "the speckle is gone from keep"


def test_update_behind_the_stream_eager_and_captured():
    """A three-frame 128x256 sequence on the tiny model, iters = 2: the occlusion mask of a bidirectional FlowStream step goes
    through MovingObjects.update (values: the forward flow) and allocates nothing.  The update, captured into ONE graph after a
    side-stream warm-up and replayed twice on copied-in inputs over poisoned buffers, gives the eager call's bits.  This exercises launches, state and capture."""
    from prior_flow_amd.modules import state_dict_shapes
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
    mo = MovingObjects(B, H, W, DEV, channels=2, min_area=2.0)
    mask = torch.zeros(B, H, W, dtype=torch.uint8, device=DEV)
    values = torch.zeros(B, 2, H, W, device=DEV)

    with torch.no_grad():
        assert stream(frames[0]) is None
        stream(frames[1])
        r = stream(frames[2])
        occ, flow = r.occ_forward.reshape(B, H, W).to(torch.uint8).contiguous(), r.forward.contiguous().clone()
        torch.cuda.synchronize()
        n0 = torch.cuda.memory_stats()["allocation.all.allocated"]
        mo.update(occ, flow)
        mo.update(occ, flow)
        assert torch.cuda.memory_stats()["allocation.all.allocated"] == n0, "an update allocated device memory"
        want = _state(mo)
        print(f"[segments] behind the stream: {int((occ != 0).sum())} occluded pixels, {int(want['count'][0])} objects of area >= 2")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            mo.update(mask, values)                                        # warm-up on the side stream
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            mo.update(mask, values)
        mask.copy_(occ)                                                    # the inputs arrive after the capture
        values.copy_(flow)
        for _ in range(2):
            for x in (mo.labels, mo.ids, mo.roots, mo.count, mo.sums, mo._t.scratch):
                x.fill_(-1)
            mo.keep.fill_(255)
            mo.table.fill_(float("nan"))
            graph.replay()
            torch.cuda.synchronize()
            assert _equal(_state(mo), want)
        assert int(want["count"][0]) == int((want["roots"][0] >= 0).sum()) or int(want["count"][0]) > mo.M
