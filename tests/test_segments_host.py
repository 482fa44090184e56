"""Connected components on the cyclic panorama, on the host: the emulation (tests/emu/pf_emu_segments.cpp over
csrc/pf_segments.h, the header the device kernels compile) against the flood-fill statement of tests/segments_ref.py, bit for bit
in every integer and within the derived float64 bound in the table; the order of the merge's unions; the properties of the
statement; planted faults; the refusals; the moving-ball scene through the Python layer."""
import numpy as np
import pytest
import torch

import segments_cases as sc
import segments_ref as sr


@pytest.fixture(scope="module")
def emu():
    return sc.emu()


def _emu_and_ref(emu, family, B, C, H, W, setting, fault=None):
    conn, poles, M, min_area = setting
    m, v = sc.mask(family, B, H, W), sc.values(B, C, H, W)
    got = sc.run(emu, m, v, conn, poles, M, min_area)
    return got, sc.reference(m, v, conn, poles, M, min_area, got["rows"], got["cols"], fault)


@pytest.mark.parametrize("B,C,H,W", sc.SWEEP)
def test_emulation_matches_the_flood_fill(emu, B, C, H, W):
    worst, runs = 0.0, 0
    for family in sc.FAMILIES:
        for setting in sc.combos(family):
            got, ref = _emu_and_ref(emu, family, B, C, H, W, setting)
            worst = max(worst, sc.against_reference(got, ref, f"{family} {B}x{C}x{H}x{W} {setting}"))
            runs += 1
            if family == "full":
                assert (got["labels"] == 1).all()
            if family == "empty":
                assert not got["labels"].any() and not got["count"].any() and (got["roots"] == -1).all() and not got["table"].any()
    print(f"[segments] emulation {B}x{C}x{H}x{W}: {runs} runs, worst table error / bound {worst:.3f}")


@pytest.mark.parametrize("family", sc.DEVICE_FAMILIES)
@pytest.mark.parametrize("case", sc.DEVICE_PATHS, ids=sc.case_id)
def test_emulation_matches_the_flood_fill_at_the_device_path_cases(emu, case, family):
    """The host twin of tests/test_hip_segments.py's cases for the device-only paths (a capped grid, a scan of several rows per
    thread, the tables at their limits), at B = 512 for twice a whole card's CUs: the restatement is held to the flood fill before
    a device is held to the restatement.  Under sc.OVERFLOWS both new tables must be full, whatever becomes of the masks."""
    B, C, H, W = sc.device_case(case)
    m, v = sc.mask(family, B, H, W), sc.values(B, C, H, W)
    worst = 0.0
    for setting in sc.device_combos(family):
        conn, poles, M, min_area = setting
        what = f"{family} {B}x{C}x{H}x{W} {setting}"
        got = sc.run(emu, m, v, conn, poles, M, min_area)
        ref = sc.reference(m, v, conn, poles, M, min_area, got["rows"], got["cols"], lab=sc.flood_fill(family, B, H, W, conn, poles))
        worst = max(worst, sc.against_reference(got, ref, what))
        if (case, family) == sc.OVERFLOWS and setting in sc.FULL_TABLES:
            print(f"[segments] {what}: survivors per image {got['count'].tolist()}")
            assert (got["count"] > M).all() and (got["roots"] >= 0).all(), f"{what}: the table is not full"
        if setting in sc.FULL_TABLES or poles:
            try:
                for seed in sc.ORDERS:
                    emu._dll.pf_emu_seg_order(seed)
                    sc.same_bits(sc.run(emu, m, v, conn, poles, M, min_area), got, f"{what} order {seed}")
            finally:
                emu._dll.pf_emu_seg_order(0)
    if family == "full":
        assert (got["labels"] == 1).all()
    print(f"[segments] emulation {B}x{C}x{H}x{W} {family}: worst table error / bound {worst:.3f}")


def test_checkerboard_counts(emu):
    """One component at 8; every pixel its own at 4; at odd W the seam joins two columns of equal parity."""
    for H, W in ((6, 10), (6, 11)):
        m = sc.mask("checker", 1, H, W)
        n8 = len(np.unique(sc.run(emu, m, None, 8, False, 8, 0.0)["labels"])) - 1
        n4 = len(np.unique(sc.run(emu, m, None, 4, False, 8, 0.0)["labels"])) - 1
        joined = sum(1 for y in range(H) if m[0, y, 0] and m[0, y, W - 1])
        assert n8 == 1 and n4 == int(m.sum()) - joined and (joined > 0) == (W % 2 == 1)


@pytest.mark.parametrize("family,B,H,W", (("serpentine", 2, 64, 128), ("spiral", 1, 130, 257), ("bernoulli_0.59", 1, 130, 257),
                                          ("bernoulli_0.41", 1, 40, 1100), ("pole_scatter", 2, 64, 128)))
def test_labels_do_not_depend_on_the_order_of_the_unions(emu, family, B, H, W):
    m = sc.mask(family, B, H, W)
    try:
        for conn, poles in ((4, False), (8, True)):
            want = sc.run(emu, m, None, conn, poles, 16, 1.0)
            for seed in (1, 2, 77, 123456789):
                emu._dll.pf_emu_seg_order(seed)
                sc.same_bits(sc.run(emu, m, None, conn, poles, 16, 1.0), want, f"{family} order {seed}")
                emu._dll.pf_emu_seg_order(0)
    finally:
        emu._dll.pf_emu_seg_order(0)


def _same_partition(a, b):
    assert ((a > 0) == (b > 0)).all()
    pairs = np.unique(np.stack([a[a > 0], b[a > 0]]), axis=1).shape[1]
    return pairs == len(np.unique(a[a > 0])) == len(np.unique(b[b > 0]))


def test_properties(emu):
    B, H, W = 1, 33, 70
    # a cyclic shift in x moves the components and changes nothing else
    for family in ("bernoulli_0.5", "seam_blob", "spiral"):
        m = sc.mask(family, B, H, W)
        for conn in (4, 8):
            a = sc.run(emu, m, None, conn, False, 1024, 0.0)
            for s in (1, 13, W - 1):
                b = sc.run(emu, np.roll(m, s, axis=2), None, conn, False, 1024, 0.0)
                back = np.roll(b["labels"], -s, axis=2)
                assert _same_partition(a["labels"][0], back[0]), (family, conn, s)
                # renumbered by the root's shifted index: the label is the smallest index of the shifted component
                yy, xx = np.divmod(back[0][back[0] > 0] - 1, W)
                assert (b["labels"][0][yy, xx] == back[0][back[0] > 0]).all()
                assert (a["count"] == b["count"]).all() and sorted(a["sums"][0, :, 1]) == sorted(b["sums"][0, :, 1])
    # min_area = 0 and room for everything: every component is kept
    m = sc.mask("bernoulli_0.3", B, H, W)
    full = sc.run(emu, m, None, 4, False, 4096, 0.0)
    n = len(np.unique(full["labels"])) - 1
    assert full["count"][0] == n <= 4096 and (full["keep"] == (m != 0)).all() and ((full["ids"] > 0) == (m != 0)).all()
    assert sorted(np.unique(full["ids"]))[-1] == n and (full["roots"][0, :n] == np.unique(full["labels"])[1:] - 1).all()
    # more survivors than rows: count says so, ids beyond the cap are 0, keep still holds them
    few = sc.run(emu, m, None, 4, False, 5, 0.0)
    assert few["count"][0] == n > 5 and few["ids"].max() == 5 and (few["keep"] == (m != 0)).all()
    assert ((few["ids"] == 0) & (m != 0)).any() and (few["ids"][full["ids"] > 5] == 0).all() and (few["ids"][full["ids"] <= 5] == full["ids"][full["ids"] <= 5]).all()
    # the same blob is worth less near a pole
    H, W = 64, 128
    blob = np.zeros((1, H, W), np.uint8)
    blob[0, 30:34, 10:14] = 1
    blob[0, 2:6, 60:64] = 1
    t = sc.run(emu, blob, None, 8, False, 4, 0.0)["table"][0]
    assert t[0, 1] == t[1, 1] == 16 and t[0, 0] < 0.25 * t[1, 0] and abs(t[1, 0] - 16) < 0.05
    assert abs(t[0, 0] - sum(4 * np.cos((0.5 - (y + 0.5) / H) * np.pi) for y in range(2, 6))) < 1e-3
    # the centroid of a blob across the seam lies on the seam (x = -1/2 or W - 1/2), not at W/2
    seam = np.zeros((1, H, W), np.uint8)
    seam[0, 20:30, :3] = 1
    seam[0, 20:30, W - 3:] = 1
    t = sc.run(emu, seam, None, 8, False, 4, 0.0)
    assert t["count"][0] == 1 and min(abs(t["table"][0, 0, 2] + 0.5), abs(t["table"][0, 0, 2] - (W - 0.5))) < 1e-3
    assert abs(t["table"][0, 0, 3] - 24.5) < 0.2 and t["table"][0, 0, 4] > 0.95
    # a ring around the sphere has no direction: the resultant is small
    ring = np.zeros((1, H, W), np.uint8)
    ring[0, 31:33] = 1
    assert sc.run(emu, ring, None, 4, False, 4, 0.0)["table"][0, 0, 4] < 1e-3


# which case shows which planted fault: (family, (B, C, H, W), (connectivity, poles, max_objects, min_area))
CATCHES = {
    "no_seam": ("seam_blob", (2, 4, 17, 37), (4, False, 8, 0.0)),
    "no_seam_diagonal": ("seam_diag", (2, 4, 17, 37), (8, False, 64, 1.5)),
    "no_corner_diagonal": ("corner_diag", (2, 3, 64, 128), (8, False, 64, 1.5)),
    "max_label": ("bernoulli_0.3", (1, 3, 6, 10), (4, False, 8, 0.0)),
    "four_for_eight": ("checker", (1, 3, 6, 10), (8, False, 64, 1.5)),
    "area_no_cos": ("bernoulli_0.5", (2, 4, 17, 37), (8, False, 64, 1.5)),
    "ids_off_by_one": ("vstripes", (1, 3, 6, 10), (4, False, 8, 0.0)),
    "count_clipped": ("checker", (2, 4, 17, 37), (4, False, 8, 0.0)),
    "poles_ignored": ("pole_scatter", (2, 4, 17, 37), (8, True, 64, 1.5)),
    "nan_counted": ("full", (2, 4, 17, 37), (8, False, 64, 1.5)),
}


@pytest.mark.parametrize("fault", sr.FAULTS)
def test_planted_faults_are_caught(emu, fault):
    family, (B, C, H, W), setting = CATCHES[fault]
    got, good = _emu_and_ref(emu, family, B, C, H, W, setting)
    sc.against_reference(got, good, f"{family} without the fault")
    _, bad = _emu_and_ref(emu, family, B, C, H, W, setting, fault)
    with pytest.raises(AssertionError):
        sc.against_reference(got, bad, fault)


def test_refusals(emu):
    from prior_flow_amd._lib import PfError
    from prior_flow_amd.segments import MovingObjects, label_components
    B, H, W = 2, 6, 10
    m = torch.from_numpy(sc.mask("bernoulli_0.5", B, H, W).copy())
    mo = MovingObjects(B, H, W, "cpu", channels=1, lib=emu)
    v = torch.zeros(B, 1, H, W)
    bad = [lambda: mo.update(m, None), lambda: mo.update(m.float(), v), lambda: mo.update(m[:, :, :5], v), lambda: mo.update(m, v.double()),
           lambda: mo.update(m.transpose(1, 2).contiguous().transpose(1, 2), v), lambda: mo.update(mo.keep, v),
           lambda: mo.update_parallax(m, v, v, v[:, 0]), lambda: MovingObjects(B, H, W, "cpu", max_objects=0, lib=emu),
           lambda: MovingObjects(B, H, W, "cpu", max_objects=4097, lib=emu), lambda: MovingObjects(B, H, W, "cpu", min_area=-1.0, lib=emu),
           lambda: MovingObjects(B, H, W, "cpu", min_area=float("nan"), lib=emu), lambda: MovingObjects(B, H, W, "cpu", connectivity=6, lib=emu),
           lambda: MovingObjects(B, H, W, "cpu", channels=5, lib=emu), lambda: MovingObjects(0, H, W, "cpu", lib=emu),
           lambda: MovingObjects(B, H, W, "cpu"), lambda: label_components(m), lambda: label_components(m, connectivity=5, lib=emu),
           lambda: label_components(m, out=torch.zeros(B, H, W), lib=emu), lambda: emu.seg_scratch_bytes(1, 1 << 15, 1 << 15)]
    for i, f in enumerate(bad):
        with pytest.raises(PfError):
            f()
        assert not mo.labels.any() and not mo.ids.any() and not mo.sums.any(), i
    # the C checks behind the wrappers: scratch too small, aliasing, a misaligned table
    rows, cols = torch.zeros(H, 2), torch.zeros(W, 2)
    emu.seg_tables(rows, cols)
    labels = torch.zeros(B, H, W, dtype=torch.int32)
    with pytest.raises(PfError):
        emu.seg_label(m, rows, labels, torch.zeros(4, dtype=torch.int64), 8, False)
    with pytest.raises(PfError):
        emu.seg_label(m, rows, labels, mo._t.scratch, 7, False)
    ids, count, table = mo.update(m, v)
    assert torch.equal(label_components(m, lib=emu), mo.labels) and int(count.sum()) > 0


@pytest.mark.parametrize("H,W,theta", sc.BALL_SCENES)
def test_the_restatement_finds_the_ball(emu, H, W, theta):
    """The scene's parameters are held to this check on the host before any device sees them: the flood fill and the emulation
    (through MovingObjects.update_parallax) both find the ball."""
    from prior_flow_amd.segments import MovingObjects
    s = sc.ball_scene(H, W, theta)
    mo = MovingObjects(1, H, W, "cpu", channels=3, lib=emu)
    ids, count, table = mo.update_parallax(*(torch.from_numpy(s[k]) for k in ("moving", "flow", "rigid_flow", "inv_depth")))
    v = mo.values.numpy()
    ref = sc.reference(s["moving"], v, 8, False, 64, 4.0, mo.rows.numpy(), mo.cols.numpy())
    sc.ball_check(ref["table"], ref["count"], s, W, f"flood fill {H}x{W}")
    sc.ball_check(table.numpy(), count.numpy(), s, W, f"emulation {H}x{W}")
    got = dict(labels=mo.labels.numpy(), ids=ids.numpy(), keep=mo.keep.numpy(), roots=mo.roots.numpy(), count=count.numpy(),
               sums=mo.sums.numpy(), table=table.numpy())
    sc.against_reference(got, ref, f"ball {H}x{W}")
    assert int(mo.keep.sum()) < int(s["moving"].sum()), "the speckle is gone from keep"
