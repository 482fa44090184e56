"""Object tracks on the host: the emulation (tests/emu/pf_emu_tracker.cpp over csrc/pf_tracker.h, the header
the device kernels compile) against the numpy / Python statement of tests/tracker_ref.py, bit for bit in every integer and within
the derived bound in step and path; the order of the votes; the properties of the statement over three pushes; reset; planted
faults; the refusals; the four-frame moving-ball scene through the Python layer."""
import ctypes

import numpy as np
import pytest
import torch

import segments_cases as sc
import tracker_cases as tc
import tracker_ref as tr


@pytest.fixture(scope="module")
def emu():
    return tc.emu()


def _objects(emu, p, M, min_area):
    H, W = p["masks"][0].shape[1:]
    rows, cols = sc.tables(emu, H, W)
    return rows, tuple(tc.objects(lab, rows, cols, M, min_area) for lab in p["labels"])


def _check_pair(emu, family, B, H, W, M, min_area, direction, fault=None):
    p = tc.pair(family, B, H, W)
    rows, (o0, o1) = _objects(emu, p, M, min_area)
    g1, g2, (r1, n1), (r2, n2) = tc.run_pair(emu, p, o0, o1, rows, direction, M, fault=fault)
    what = f"{family} {B}x{H}x{W} M={M} {direction}"
    return max(tc.against_reference(g1, r1, n1, what + " push 1"), tc.against_reference(g2, r2, n2, what + " push 2")), o0, o1, g2


@pytest.mark.parametrize("B,H,W", tc.SHAPES)
def test_emulation_matches_the_reference(emu, B, H, W):
    worst, runs, over = 0.0, 0, False
    for family in tc.FAMILIES:
        for M, min_area in tc.SETTINGS:
            for direction in tc.DIRECTIONS:
                w, o0, o1, _ = _check_pair(emu, family, B, H, W, M, min_area, direction)
                worst, runs = max(worst, w), runs + 1
                over |= bool((o0[1] > M).any() or (o1[1] > M).any())
    if H * W >= 17 * 37:
        assert over, "count > M does not occur in this sweep"
    print(f"[tracker] emulation {B}x{H}x{W}: {runs} pairs, worst step / path error / bound {worst:.3f}")


@pytest.mark.parametrize("family", tc.DEVICE_FAMILIES)
@pytest.mark.parametrize("case", tc.DEVICE_PATHS, ids=sc.case_id)
def test_emulation_matches_the_reference_at_the_device_path_cases(emu, case, family):
    """The host twin of tests/test_hip_tracker.py's cases for the device-only paths (a capped vote grid, the table at
    PF_TRK_MAX_OBJECTS), at B = 512 for twice a whole card's CUs.  At the product size the full table really is full."""
    B, H, W = tc.device_case(case)
    small, full = tc.device_pair(family, B, H, W)
    rows, cols = sc.tables(emu, H, W)
    worst, runs = 0.0, 0
    for M, min_area in tc.DEVICE_SETTINGS:
        o0, o1 = (tc.objects(lab, rows, cols, M, min_area) for lab in small["labels"])
        if (case, family) == tc.OVERFLOWS and (M, min_area) == tc.FULL_TABLE:
            print(f"[tracker] {family} {B}x{H}x{W} M={M}: objects per image {o0[1].tolist()} and {o1[1].tolist()}")
            assert (o0[1] > M).all() and (o1[1] > M).all(), "the table of 256 is not full in both frames"
        for direction in tc.DIRECTIONS:
            what = f"{family} {B}x{H}x{W} M={M} {direction}"
            g1, g2, (r1, n1), (r2, n2) = tc.run_pair_tiled(emu, small, full, o0, o1, rows, direction, M)
            worst = max(worst, tc.against_reference(g1, r1, n1, what + " push 1"), tc.against_reference(g2, r2, n2, what + " push 2"))
            runs += 1
            assert g2["votes"].any(), what
    print(f"[tracker] emulation {B}x{H}x{W} {family}: {runs} pairs, worst step / path error / bound {worst:.3f}")


@pytest.mark.parametrize("family,B,H,W,M", (("bernoulli_0.5", 2, 64, 128, 64), ("junk", 1, 33, 70, 8), ("bernoulli_0.41", 1, 40, 1100, 200)))
def test_votes_do_not_depend_on_the_order_of_the_pixels(emu, family, B, H, W, M):
    p = tc.pair(family, B, H, W)
    rows, (o0, o1) = _objects(emu, p, M, 0.0)
    try:
        want = tc.run_pair(emu, p, o0, o1, rows, "both", M)[1]
        assert want["votes"].any()
        for seed in (1, 2, 77, 4242, 123456789):
            emu._dll.pf_emu_trk_order(seed)
            tc.same_bits(tc.run_pair(emu, p, o0, o1, rows, "both", M)[1], want, f"{family} order {seed}")
            emu._dll.pf_emu_trk_order(0)
    finally:
        emu._dll.pf_emu_trk_order(0)


def _three_pushes(emu, family, direction="both", B=1, H=33, W=70, M=64):
    """Frame 0 (everything new), frame 1 along the pair's flows, frame 0 again along the same flows the other way round."""
    p = tc.pair(family, B, H, W)
    rows, (o0, o1) = _objects(emu, p, M, 0.0)
    fp, fc, mp, mc = tc.flows(p, direction)
    t = tc.Tracker(emu, B, H, W, M)
    g1 = t.push(*o0, np.zeros((B, 2, H, W), np.float32), None, None, None, rows)
    g2 = t.push(*o1, fp, fc, mp, mc, rows)
    g3 = t.push(*o0, fc, fp, mc, mp, rows)
    return g1, g2, g3, o0, o1


@pytest.mark.parametrize("direction", tc.DIRECTIONS)
def test_properties_over_three_pushes(emu, direction):
    for family in ("static", "shift", "seam", "masked"):
        g1, g2, g3, o0, _ = _three_pushes(emu, family, direction)
        n = int(o0[1][0])
        assert n == 2 and g1["track"][0, :n].tolist() == [1, 2] and (g1["age"][0, :n] == 1).all() and not g1["origin"][0].any()
        for g, age in ((g2, 2), (g3, 3)):
            assert (g["age"][0, :n] == age).all() and (g["origin"][0, :n] == g["track"][0, :n]).all(), family
            assert sorted(g["track"][0, :n].tolist()) == [1, 2] and g["next_id"][0] == 3, family
        assert g3["track"][0, :n].tolist() == [1, 2] and (g3["fate"][0, :n] > 0).all(), family
        if family != "static":
            assert (g2["step"][0, :n] > 0).all() and (g3["path"][0, :n] > g2["path"][0, :n]).all(), family
        else:
            assert not g2["step"][0].any() and not g3["path"][0].any()
    # swap: the ids follow the blobs, not the raster order
    _, g2, g3, _, _ = _three_pushes(emu, "swap", direction)
    assert g2["track"][0, :2].tolist() == [2, 1] and g2["age"][0, :2].tolist() == [2, 2] and g2["fate"][0, :2].tolist() == [2, 1]
    assert g3["track"][0, :2].tolist() == [1, 2] and g3["age"][0, :2].tolist() == [3, 3]
    assert (g2["track_map"][0][g2["st_ids"][0] == 1] == 2).all() and (g2["track_map"][0][g2["st_ids"][0] == 0] == 0).all()
    # split: the larger piece (the second slot) inherits, the other is new and names its parent
    _, g2, g3, _, o1 = _three_pushes(emu, "split", direction)
    assert int(o1[1][0]) == 2 and o1[2][0, 1, 0] > o1[2][0, 0, 0]
    assert g2["track"][0, :2].tolist() == [2, 1] and g2["age"][0, :2].tolist() == [1, 2] and g2["origin"][0, :2].tolist() == [1, 1]
    assert g2["fate"][0, 0] == 2 and g2["next_id"][0] == 3
    # ... and going back is a merge: the absorbed piece's fate is negative
    assert g3["track"][0, 0] == 1 and g3["age"][0, 0] == 3 and g3["fate"][0, :2].tolist() == [-1, 1]
    # tie: two equal pieces, the smaller slot inherits
    _, g2, _, _, o1 = _three_pushes(emu, "tie", direction)
    assert o1[2][0, 0, 0] == o1[2][0, 1, 0] and g2["votes"][0, 0, 0] == g2["votes"][0, 0, 1] > 0
    assert g2["track"][0, :2].tolist() == [1, 2] and g2["age"][0, :2].tolist() == [2, 1] and g2["origin"][0, :2].tolist() == [1, 1]
    # merge: the larger piece's track goes on, the other is absorbed
    g1, g2, _, _, _ = _three_pushes(emu, "merge", direction)
    assert g1["track"][0, :2].tolist() == [1, 2] and g2["track"][0, 0] == 2 and g2["age"][0, 0] == 2
    assert g2["fate"][0, :2].tolist() == [-1, 1] and g2["next_id"][0] == 3
    # birth and death
    _, g2, _, _, _ = _three_pushes(emu, "birth_death", direction)
    assert g2["track"][0, :2].tolist() == [1, 3] and g2["age"][0, :2].tolist() == [2, 1] and g2["origin"][0, :2].tolist() == [1, 0]
    assert g2["fate"][0, :2].tolist() == [1, 0] and g2["next_id"][0] == 4 and g2["step"][0, 1] == 0 and g2["path"][0, 1] == 0


# which case shows which planted fault: (family, (B, H, W), (max_objects, min_area), direction)
CATCHES = {
    "no_wrap": ("seam", (2, 17, 37), (8, 0.0), "forward"),
    "truncate": ("shift", (1, 33, 70), (64, 1.5), "both"),
    "mask_ignored": ("masked", (1, 33, 70), (64, 1.5), "forward"),
    "no_transpose": ("split", (1, 33, 70), (64, 1.5), "backward"),
    "ties_largest": ("tie", (2, 17, 37), (8, 0.0), "both"),
    "row_only": ("merge", (1, 33, 70), (64, 1.5), "both"),
    "thr_max": ("split", (1, 33, 70), (64, 1.5), "forward"),
    "ids_top_down": ("static", (2, 17, 37), (8, 0.0), "forward"),
    "age_stuck": ("static", (1, 33, 70), (200, 0.0), "both"),
    "merged_lost": ("merge", (2, 64, 128), (64, 1.5), "backward"),
}


@pytest.mark.parametrize("fault", tr.FAULTS)
def test_planted_faults_are_caught(emu, fault):
    family, (B, H, W), (M, min_area), direction = CATCHES[fault]
    _check_pair(emu, family, B, H, W, M, min_area, direction)                 # the unfaulted reference passes
    with pytest.raises(AssertionError):
        _check_pair(emu, family, B, H, W, M, min_area, direction, fault)


def _python_tracker(emu, B, H, W, M=8, **kw):
    from prior_flow_amd.object_tracks import ObjectTracker
    from prior_flow_amd.segments import MovingObjects
    mo = MovingObjects(B, H, W, "cpu", max_objects=M, min_area=0.0, lib=emu)
    return mo, ObjectTracker(mo, **kw)


def _bits(tk):
    names = ("votes", "track", "age", "origin", "fate", "step", "path", "track_map", "next_id", "prev_ids", "prev_count", "prev_sums",
             "prev_track", "prev_age", "prev_path")
    return {n: getattr(tk, n).clone() for n in names}


def _equal(a, b):
    return all(torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)) for k in a)


def test_python_layer_reset_and_grids(emu):
    """grid = "second" links with the current pair's flows, grid = "first" with the pair before; a poisoned tracker after reset()
    gives a fresh tracker's bits."""
    from collections import namedtuple
    R = namedtuple("R", "forward backward occ_forward occ_backward")
    B, H, W = 2, 17, 37
    p = tc.pair("shift", B, H, W)
    t = lambda a: None if a is None else torch.from_numpy(np.array(a))       # noqa: E731
    m0, m1 = (t(m) for m in p["masks"])
    r = R(t(p["fw"]), t(p["bw"]), torch.zeros(B, H, W, dtype=torch.uint8), None)
    mo, tk = _python_tracker(emu, B, H, W, grid="second")
    mo.update(m0)
    tk.push(r)
    first = _bits(tk)
    assert first["track"][0, :2].tolist() == [1, 2] and first["next_id"].tolist() == [3, 3]
    mo.update(m1)
    track, age, track_map = tk.push(r)
    assert track[0, :2].tolist() == [1, 2] and age[0, :2].tolist() == [2, 2] and (track_map[mo.ids > 0] > 0).all()
    assert torch.equal(tk.prev_ids, mo.ids) and torch.equal(tk.prev_sums, mo.sums) and torch.equal(tk.prev_count, mo.count)
    # the same through link, and with grid = "first" one push later (the first frame's objects again: the flows arrive late)
    mo2, tk2 = _python_tracker(emu, B, H, W, grid="first")
    mo2.update(m0)
    tk2.push(r)
    mo2.update(m1)
    tk2.push(R(torch.zeros_like(r.forward), torch.zeros_like(r.backward), None, None))
    assert _equal(_bits(tk2), _bits(tk))
    # poison, reset: a fresh tracker's first push
    for n, x in _bits(tk).items():
        getattr(tk, n).fill_(float("nan") if x.dtype.is_floating_point else -1)
    tk.reset()
    mo.update(m0)
    tk.push(r)
    assert _equal(_bits(tk), first)


def test_refusals(emu):
    from collections import namedtuple
    from prior_flow_amd._lib import PfError
    from prior_flow_amd.object_tracks import ObjectTracker
    from prior_flow_amd.segments import MovingObjects
    R = namedtuple("R", "forward backward occ_forward occ_backward")
    B, H, W = 2, 6, 10
    mo, tk = _python_tracker(emu, B, H, W)
    mo.update(torch.from_numpy(sc.mask("bernoulli_0.5", B, H, W).copy()))
    f, m = torch.zeros(B, 2, H, W), torch.zeros(B, H, W, dtype=torch.uint8)
    bad = [lambda: tk.link(None, None), lambda: tk.link(f.double(), None), lambda: tk.link(f[:, :1].contiguous(), None),
           lambda: tk.link(f, f[:, :, :3]), lambda: tk.link(f, None, m.int()), lambda: tk.link(f, None, None, m[:1]),
           lambda: tk.link(f.numpy(), None), lambda: tk.push(R(f, None, None, None)), lambda: tk.push(f),
           lambda: tk.link(f, None, tk.mask_prev), lambda: tk.link(tk.flow_cur, None), lambda: tk.push(R(f, tk.flow_prev, None, None)),
           lambda: ObjectTracker(MovingObjects(B, H, W, "cpu", max_objects=257, lib=emu)), lambda: ObjectTracker(mo, min_overlap=0.0),
           lambda: ObjectTracker(mo, min_overlap=1.5), lambda: ObjectTracker(mo, min_overlap=float("nan")),
           lambda: ObjectTracker(mo, grid="third"), lambda: ObjectTracker(None)]
    for i, fn in enumerate(bad):
        with pytest.raises(PfError):
            fn()
        assert not any(x.any() for k, x in _bits(tk).items() if k != "next_id") and (tk.next_id == 1).all(), i
    # the C checks, with live host pointers: nothing is launched
    d, M = emu._dll, 8
    i64, i32, f32 = (lambda n: torch.zeros(n, dtype=torch.int64)), (lambda n: torch.zeros(n, dtype=torch.int32)), (lambda n: torch.zeros(n))
    P = lambda x: ctypes.c_void_p(x.data_ptr())                              # noqa: E731
    N = B * H * W
    votes, prev, ids, flow, rows = i64(B * M * M + 1), i32(N), i32(N), f32(2 * N), f32(2 * H)
    vote = lambda **k: d.pf_trk_vote(*[k.get(n, v) for n, v in (("prev", P(prev)), ("ids", P(ids)), ("fp", P(flow)), ("fc", None),   # noqa: E731
                                                                  ("mp", None), ("mc", None), ("rows", P(rows)), ("votes", P(votes)),
                                                                  ("B", B), ("H", H), ("W", W), ("M", M))], None)
    assert vote() == 0
    assert vote(fp=None) == -1 and vote(prev=None) == -1 and vote(rows=None) == -1 and vote(votes=None) == -1
    assert vote(votes=ctypes.c_void_p(votes.data_ptr() + 4)) == -1 and vote(votes=P(flow)) == -1 and vote(fc=P(flow)) == 0
    assert vote(B=0) == -2 and vote(H=0) == -2 and vote(B=65536) == -2 and vote(H=1 << 15, W=1 << 15) == -2
    assert vote(M=0) == -2 and vote(M=257) == -2
    assert d.pf_trk_begin(None, B, M, None) == -1 and d.pf_trk_begin(P(votes), B, 300, None) == -2
    cnt, sums, st = i32(B), i64(B * M * 10), [i32(B), i64(B * M * 10), i32(B * M), i32(B * M), f32(B * M), i32(B)]
    outs = [i32(B * M) for _ in range(4)] + [f32(B * M), f32(B * M)]

    def match(mo_=0.25, n_dir=1, **k):
        a = [P(votes), P(cnt), P(sums)] + [P(x) for x in st] + [P(x) for x in outs]
        for i, v in k.items():
            a[int(i[1:])] = v
        return d.pf_trk_match(*a, B, M, n_dir, ctypes.c_float(mo_), None)

    assert match() == 0
    assert match(0.0) == -1 and match(1.25) == -1 and match(float("nan")) == -1 and match(-0.5) == -1 and match(1.0) == 0
    assert match(n_dir=0) == -1 and match(n_dir=3) == -1 and match(a9=None) == -1 and match(a4=P(sums)) == -1 and match(a10=P(outs[0])) == -1
    assert match(a2=ctypes.c_void_p(sums.data_ptr() + 4)) == -1
    tm, si = i32(N), i32(N)
    assert d.pf_trk_paint(P(ids), P(outs[0]), P(tm), P(si), B, H, W, M, None) == 0
    assert d.pf_trk_paint(P(ids), P(outs[0]), P(ids), P(si), B, H, W, M, None) == -1
    assert d.pf_trk_paint(P(ids), P(outs[0]), P(tm), None, B, H, W, M, None) == -1
    assert d.pf_trk_paint(P(ids), P(outs[0]), P(tm), P(si), B, H, W, 0, None) == -2


def test_built_library_refuses_without_a_gpu():
    """The product's entry points answer their refusals before any launch, so they can be asked here."""
    import __graft_entry__ as ge
    d = ctypes.CDLL(ge.build_hip())
    buf = [ctypes.cast((ctypes.c_longlong * 64)(), ctypes.c_void_p) for _ in range(4)]
    assert d.pf_trk_begin(None, 1, 8, None) == -1 and d.pf_trk_begin(buf[0], 1, 257, None) == -2
    assert d.pf_trk_vote(buf[0], buf[1], None, None, None, None, buf[2], buf[3], 1, 2, 2, 2, None) == -1
    assert d.pf_trk_vote(buf[0], buf[1], buf[2], None, None, None, buf[2], buf[3], 1, 0, 2, 2, None) == -2
    assert d.pf_trk_paint(buf[0], buf[1], buf[0], buf[2], 1, 2, 2, 2, None) == -1


@pytest.mark.parametrize("H,W,theta", sc.BALL_SCENES)
def test_the_emulation_tracks_the_ball(emu, H, W, theta):
    """The scene's parameters are held to this check on the host before any device sees them."""
    seq = tc.ball_sequence(H, W, theta)
    tc.ball_track_check(tc.ball_track(seq, H, W, "cpu", emu), seq, f"emulation {H}x{W}")
