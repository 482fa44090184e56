"""The 360-degree training augmentation without a GPU: the numpy restatement (tests/augment_ref.py) and the
host emulation of pf_augment_360 / pf_augment_convert (tests/emu/pf_emu_augment.cpp over csrc/pf_augment.h, the header the
device kernels compile) against PIL's stored single operations and the reference's stored FlowAugmentor_360 runs
(tests/golden/augment_360.npz, written by tests/gen_golden_augment.py); the sampler; hand-made geometry; the argument checks.

Bars: brightness / contrast / saturation and HSV -> RGB alone bit for bit; anything containing RGB -> HSV under the cap (at most
0.5 % of bytes differ, a lone hue step by at most 7 levels, a chain by at most 28); flow and valid bit for bit.
Measured here (restatement and emulation alike): 0 differing bytes on every stored single operation, on RGB -> HSV, on the hue
step alone and on all nine stored reference runs -- Pillow's 8-bit HSV is reproduced exactly, so the host checks below assert
equality, which is stricter than the cap.
"""
import ctypes
import shutil

import numpy as np
import pytest
import torch

import augment_cases as ac
import augment_ref as ar


@pytest.fixture(scope="module")
def emu():
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    import __graft_entry__ as ge
    from prior_flow_amd import _lib
    so = ge.build_emu_augment()
    return _lib.PfLib(so, require_cuda=False, optional=tuple(n for n in _lib.EXPORTS if not n.startswith("pf_augment")))


@pytest.fixture(scope="module")
def gold():
    return ac.golden()


def _emu_colour(emu, img, params):
    """The colour step of the emulation on one image (both inputs the same image: the stacked mean is the image's own)."""
    got = ac.run(emu, img[None], img[None], np.zeros(img.shape[:2] + (2,), np.float32)[None], params)
    assert np.array_equal(got[0], got[1])
    return got[0][0].transpose(1, 2, 0)


# ---- bar 1: single operations bit for bit ------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", [0, 1, 2])
def test_single_operations_are_pil_bit_for_bit(emu, gold, op):
    fn = (ar.brightness, ar.contrast, ar.saturation)[op]
    for k, img in enumerate(gold["op_in"]):
        for j, f in enumerate(ac.OP_FACTORS):
            want = gold["op_out"][k, op, j]
            assert np.array_equal(fn(img, f), want), ("restatement", op, k, f)
            assert np.array_equal(_emu_colour(emu, img, ac.one_op_params(op, f)), want), ("emulation", op, k, f)


def test_hsv_conversions_are_pil_bit_for_bit(emu, gold):
    """HSV -> RGB alone is bar 1; RGB -> HSV comes out exact as well (bar 2 only asks for the cap)."""
    assert np.array_equal(ar.hsv_to_rgb(gold["hsv_back_in"]), gold["hsv_back_out"])
    assert np.array_equal(ar.rgb_to_hsv(gold["hsv_in"]), gold["hsv_out"])
    for src, want, to_rgb in ((gold["hsv_back_in"], gold["hsv_back_out"], True), (gold["hsv_in"], gold["hsv_out"], False)):
        out = torch.zeros(src.shape, dtype=torch.uint8)
        emu.augment_convert(torch.from_numpy(np.ascontiguousarray(src)), out, to_rgb)
        assert np.array_equal(out.numpy(), want), to_rgb


def test_hue_step_alone(emu, gold):
    for k, img in enumerate(gold["op_in"]):
        for j, s in enumerate(ac.HUE_SHIFTS):
            want = gold["hue_out"][k, j]
            for who, got in (("restatement", ar.hue(img, s)), ("emulation", _emu_colour(emu, img, ac.one_op_params(3, shift=s)))):
                share, worst = ac.image_diff(got, want)
                print(f"hue step alone, {who}, image {k}, shift {s}: share {share:.2e}, worst {worst:.0f}")
                assert share <= ac.CAP_SHARE and worst <= ac.CAP_HUE
                assert share == 0.0


def test_hue_factor_to_shift():
    from prior_flow_amd.augment import hue_shift
    assert [hue_shift(f) for f in (0.0, 0.1, -0.1, 0.5 / 3.14, -0.5 / 3.14, 1 / 255, -1 / 255)] == [0, 25, 231, 40, 216, 1, 255]
    assert ar.hue_shift(-0.1) == 231


# ---- bars 2, 3, 5: the stored reference runs through the sampler -------------------------------------------------------------
def test_fixture_covers_the_required_features():
    seen = set()
    for case in ac.CASES:
        have = ac.features(ac.case_params(case).row(0), *case[1])
        assert set(case[5]) <= have, (case[0], have)
        if not case[4]:
            seen |= have
    assert set(ac.REQUIRED) <= seen


@pytest.mark.parametrize("case", ac.CASES, ids=[c[0] for c in ac.CASES])
def test_stored_reference_runs(emu, gold, case):
    """sample_params_360 with the case's seed, through the restatement and the emulation, gives the reference's outputs: images
    under the cap (measured: equal), flow and valid bit for bit; for the identity cases image 1 and everything of image 2
    outside the rectangles is the rolled input."""
    name, (H, W), seed, asym_roll, identity, _ = case
    img, flow = ac.case_inputs(gold, case)
    p = ac.case_params(case)
    row = p.row(0)
    w1, w2, wf, wv = ac.case_expected(gold, case)
    with np.errstate(invalid="ignore"):
        ref = ar.augment_sample(img[0], img[1], flow, row)
    got = [o[0] for o in ac.run(emu, img[:1], img[1:], flow[None], p)]
    for who, (g1, g2, gf, gv) in (("restatement", ref), ("emulation", got)):
        share, worst = ac.image_diff(np.stack([g1, g2]), np.stack([w1, w2]))
        print(f"case {name}, {who}: share of differing bytes {share:.2e} (stored for the restatement: {float(gold[name + '_share']):.2e}),"
              f" worst {worst:.0f}")
        assert share <= ac.CAP_SHARE and worst <= ac.CAP_CHAIN
        assert share == 0.0
        if wf is not None:
            assert ac.same_flow(gf, wf), (name, who)
            assert np.array_equal(gv, wv), (name, who)
    assert ac.same_flow(got[2], ref[2]) and np.array_equal(got[3], ref[3])
    if identity:
        inside = np.zeros((H, W), bool)
        for x0, y0, dx, dy in row["rects"]:
            inside[y0:y0 + dy, x0:x0 + dx] = True
        inside = np.roll(inside, row["r2"], axis=1)
        assert np.array_equal(got[0], np.roll(img[0], row["r1"], axis=1).transpose(2, 0, 1))
        assert np.array_equal(got[1][:, ~inside], np.roll(img[1], row["r2"], axis=1).transpose(2, 0, 1)[:, ~inside])
        assert inside.any() and len(np.unique(got[1][:, inside], axis=1).T) == 1      # one mean colour for both rectangles


# ---- bar 4: hand-made geometry ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ac.SIZES, ids=ac.tag)
def test_hand_made_geometry(emu, gold, size):
    H, W = size
    img, flow = gold["smooth_" + ac.tag(size)], gold["flow_" + ac.tag(size)]
    mean = (img[1].reshape(-1, 3).astype(np.int64).sum(axis=0) // (H * W)).astype(np.float32)
    for what, rects, r1, r2 in ac.hand_cases(H, W):
        p = ac.hand_params(H, W, rects, r1, r2)
        g1, g2, gf, gv = (o[0] for o in ac.run(emu, img[:1], img[1:], flow[None], p))
        want2 = img[1].astype(np.float32)
        for x0, y0, dx, dy in rects:
            want2[y0:y0 + dy, x0:x0 + dx] = mean
        q = r1 if r2 is None else r2
        assert np.array_equal(g1, np.roll(img[0], r1, axis=1).transpose(2, 0, 1)), what
        assert np.array_equal(g2, np.roll(want2, q, axis=1).transpose(2, 0, 1)), what
        with np.errstate(invalid="ignore"):
            ref = ar.augment_sample(img[0], img[1], flow, p.row(0))
        assert ac.same_flow(gf, ref[2]) and np.array_equal(gv, ref[3]), what
        assert np.array_equal(gv == 0, ~(np.abs(gf[0]) < 1000) | ~(np.abs(gf[1]) < 1000)), what
    assert (gv == 0).any() and np.isnan(gf).any()


def test_odd_shape_against_the_restatement(emu):
    """5 x 7: H * W is no multiple of 4 (the device's contrast pass then has a tail; tests/test_hip_augment.py runs the same case)."""
    i1, i2, fl, p = ac.small_odd_batch()
    got = ac.run(emu, i1, i2, fl, p)
    for b in range(i1.shape[0]):
        with np.errstate(invalid="ignore"):
            want = ar.augment_sample(i1[b], i2[b], fl[b], p.row(b))
        assert ac.image_diff(np.stack([got[0][b], got[1][b]]), np.stack(want[:2])) == (0.0, 0.0), b
        assert ac.same_flow(got[2][b], want[2]) and np.array_equal(got[3][b], want[3]), b


@pytest.mark.parametrize("shape", ac.CAPPED, ids=lambda s: "x".join(map(str, s)))
def test_capped_shapes_against_the_restatement(emu, shape):
    """The host twin of the device's capped-grid cases (tests/test_hip_augment.py): the emulation equals the restatement on every
    byte (no hue step in these chains), and at H = 514 the content is such that the rows of the contrast pass's second trip move
    int(mean + 0.5): the restatement's images with the mean of the shortened sum differ from the right ones."""
    B, H, W = shape
    i1, i2, fl, p, row0 = ac.capped_batch(shape)
    got = ac.run(emu, i1, i2, fl, p)
    for b in range(B):
        row = p.row(b)
        with np.errstate(invalid="ignore"):
            want = ar.augment_sample(i1[b], i2[b], fl[b], row)
        assert ac.image_diff(np.stack([got[0][b], got[1][b]]), np.stack(want[:2])) == (0.0, 0.0), b
        assert ac.same_flow(got[2][b], want[2]) and np.array_equal(got[3][b], want[3]), b
        assert ac.CAPPED_RECT in row["rects"] and "seam" in ac.features(row, H, W)
    if row0 < H:
        full, short = ac.contrast_means(i1[0], i2[0], row0)
        print(f"{H}x{W}: int(mean + 0.5) of the stacked pair {full}, without the sum of rows {row0}..{H - 1}: {short}")
        assert (full, short) == (101, 100)
        s = p.row(0)["set_a"]
        assert not p.row(0)["asym_colour"] and s["order"][:2] == [0, 1] and s["fb"] == 1.0 and s["fc"] != 1.0
        right, wrong = (ar.contrast(i1[0], s["fc"], m) for m in (full, short))
        assert np.array_equal(right, ar.jitter([i1[0], i2[0]], [0, 1, 4, 4], s["fb"], s["fc"], s["fs"], 0)[0])
        share = float((right[:row0] != wrong[:row0]).mean())
        print(f"bytes of rows 0..{row0 - 1} after the contrast step that the shortened sum changes: {share:.1%}")
        assert share > 0.1


def test_untrusted_rows_stay_inside_the_maps(emu, gold):
    """Rolls of many widths, rectangles that start outside or have no area, unknown operations: reduced, dropped, skipped."""
    H, W = ac.SIZES[0]
    img, flow = gold["smooth_64x128"], gold["flow_64x128"]
    from prior_flow_amd import augment as ag
    p = ag.AugmentParams(1).set_rects(0, [(W, 0, 10, 10), (5, 5, 0, 7)]).set_roll(0, 5 * W + 3)
    p.set_colour(0, (9, -1, 77, 4), 1.3, 0.7, 1.2, shift=9)
    with pytest.raises(ag.PfError):
        p.validate(H, W)
    g1, g2, _, _ = (o[0] for o in ac.run(emu, img[:1], img[1:], flow[None], p))
    assert np.array_equal(g1, np.roll(img[0], 3, axis=1).transpose(2, 0, 1))
    assert np.array_equal(g2, np.roll(img[1], 3, axis=1).transpose(2, 0, 1))


# ---- bar 5: the sampler -----------------------------------------------------------------------------------------------------
def test_sampler_is_deterministic_and_in_range():
    from prior_flow_amd import augment as ag
    H, W = 72, 150
    draw = lambda s, **kw: ag.sample_params_360(4, H, W, np.random.RandomState(s), torch.Generator().manual_seed(s), **kw)  # noqa: E731
    assert draw(7).equal(draw(7)) and not draw(7).equal(draw(8))
    rng, gen = np.random.RandomState(123), torch.Generator().manual_seed(123)
    n, B = 0, 250
    seen = set()
    m = int(np.round(0.2 * W))
    lo, hi = np.float32(0.6), np.float32(1.4)
    while n < 10000:
        p = ag.sample_params_360(B, H, W, rng, gen, asymmetric_rotaton_aug_prob=0.3).validate(H, W)
        for b in range(B):
            row = p.row(b)
            seen |= ac.features(row, H, W)
            for s in (row["set_a"], row["set_b"]):
                assert sorted(s["order"]) == [0, 1, 2, 3]
                assert all(lo <= np.float32(s[k]) <= hi for k in ("fb", "fc", "fs"))
                assert s["shift"] <= 40 or s["shift"] >= 216                  # trunc(255 h), |h| <= 0.5 / 3.14
            assert len(row["rects"]) <= 2
            for x0, y0, dx, dy in row["rects"]:
                assert 0 <= x0 < W and 0 <= y0 < H and 50 <= dx < 100 and 50 <= dy < 100
            assert -m <= row["r1"] < m and -m <= row["r2"] < m
            assert row["asym_rot"] or row["r1"] == row["r2"]
        n += B
    assert set(ac.REQUIRED) <= seen
    # the shares of the reference's probabilities (0.2, 0.5, 0.5), loosely: 10 000 draws
    q = ag.sample_params_360(10000, H, W, np.random.RandomState(5), torch.Generator().manual_seed(5))
    asym = (q.words[:, 0] & 1).mean()
    assert 0.17 < asym < 0.23 and 0.46 < (q.words[:, 1] > 0).mean() < 0.54 and not (q.words[:, 0] & 2).any()


def test_what_is_not_built_is_refused():
    from prior_flow_amd import augment as ag
    rng, gen = np.random.RandomState(0), torch.Generator().manual_seed(0)
    for kw in (dict(do_flip=True), dict(resize_size=(256, 512)), dict(crop_size=(10, 10)), dict(v_flip_prob=0.1)):
        with pytest.raises(ag.PfError):
            ag.sample_params_360(1, 64, 128, rng, gen, **kw)
    for name in ("FlowAugmentor", "SparseFlowAugmentor_360", "FlowAugmentor_360_ortho"):
        assert not hasattr(ag, name)
    with pytest.raises(ag.PfError):
        ag.DeviceAugmentor360(1, 64, 128, "cpu")
    with pytest.raises(ag.PfError):
        ag.AugmentParams(1).set_rects(0, [(0, 0, 1, 1)] * 3)


def test_table_layout_mirrors_the_header():
    import os
    import re
    from prior_flow_amd import _lib, augment as ag
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = dict(re.findall(r"#define PF_AUG_(\w+) (\d+)", open(os.path.join(root, "prior-flow_amd", "csrc", "pf_augment.h")).read()))
    d = {k: int(v) for k, v in d.items()}
    assert (d["ROW"], d["MODE"], d["NRECT"], d["R1"], d["R2"], d["RECT"], d["SET_A"], d["SET_B"]) == \
        (ag.ROW, ag._MODE, ag._NRECT, ag._R1, ag._R2, ag._RECT, ag._SET_A, ag._SET_B)
    assert (d["ASYM_COLOUR"], d["ASYM_ROLL"]) == (ag.ASYM_COLOUR, ag.ASYM_ROLL)
    assert [d["OP_" + n] for n in ("BRIGHTNESS", "CONTRAST", "SATURATION", "HUE", "NONE")] == \
        [ag.OP_BRIGHTNESS, ag.OP_CONTRAST, ag.OP_SATURATION, ag.OP_HUE, ag.OP_NONE] == [ar.OP_BRIGHTNESS, ar.OP_CONTRAST, ar.OP_SATURATION, ar.OP_HUE, 4]
    assert ag.ROW == _lib.AUG_ROW_WORDS and "PF_AUG_ROW_WORDS 32" in open(os.path.join(root, "include", "priorflow_hip.h")).read()


# ---- the entry points' argument checks (before any launch: the product's library, no GPU needed) ------------------------------
def test_argument_checks_of_the_entry_points():
    import __graft_entry__ as ge
    dll = ctypes.CDLL(ge.build_hip())
    dll.pf_augment_scratch_bytes.restype = ctypes.c_long
    assert dll.pf_augment_scratch_bytes(3) == 3 * 8 * 8 and dll.pf_augment_scratch_bytes(0) < 0
    p = ctypes.c_void_p
    dll.pf_augment_360.argtypes = [p] * 9 + [ctypes.c_long] + [ctypes.c_int] * 3 + [p]
    a = [0x1000 * (k + 1) for k in range(9)]
    assert dll.pf_augment_360(*([None] + a[1:]), 64, 1, 64, 128, None) == -1
    assert dll.pf_augment_360(*a, 63, 1, 64, 128, None) == -1                         # scratch too small
    assert dll.pf_augment_360(*(a[:5] + [a[4]] + a[6:]), 64, 1, 64, 128, None) == -1   # image1 == image2
    assert dll.pf_augment_360(*(a[:8] + [a[8] + 4]), 64, 1, 64, 128, None) == -1       # scratch not 8-byte aligned
    for B, H, W in ((0, 64, 128), (65536, 64, 128), (1, 1, 128), (1, 64, 1), (1, 1 << 15, 1 << 15)):
        assert dll.pf_augment_360(*a, 1 << 30, B, H, W, None) == -2, (B, H, W)
    dll.pf_augment_convert.argtypes = [p, p, ctypes.c_long, ctypes.c_int, p]
    assert dll.pf_augment_convert(None, a[0], 4, 0, None) == -1 and dll.pf_augment_convert(a[0], a[0], 4, 0, None) == -1
    assert dll.pf_augment_convert(a[0], a[1], 4, 2, None) == -1 and dll.pf_augment_convert(a[0], a[1], 0, 0, None) == -2
