"""Depth along the trajectory on the host: the emulation of pf_reproj_project / pf_zsplat_front / accumulate /
resolve / pf_depth_update (tests/emu/pf_emu_reproject.cpp compiles csrc/pf_reproject.h, the file the device kernels compile) and
the Python layer (prior_flow_amd.reproject) against the restatement (tests/reproject_ref.py): the projection under the float64
bound derived there, the z-splat bit for bit, the update within a few U; the restatement itself against the truth of the analytic
scenes; order and state; the seeded faults; the refusals.

Figures of the restatement (printed by the tests, quoted in DESIGN.md section 23): the worst relative depth error on the convex
scene is TRUTH_REF per size and the emulation and the device are held to twice that; the filter's ratio is FILTER_REF."""
import ctypes

import numpy as np
import pytest
import torch

import egomotion_cases as ec
import egomotion_ref as er
import epipolar_cases as pc
import epipolar_ref as pr
import reproject_cases as rc
import reproject_ref as rr

bits = rc.bits
U = rr.U


@pytest.fixture(scope="module")
def emu():
    return rc.emu()


# ---- project ---------------------------------------------------------------------------------------------------------------------
def project_inputs(B, H, W, seed):
    rng = np.random.default_rng(seed)
    d = np.exp2(rng.uniform(-4, 1, (B, H, W))).astype(np.float32)
    d[:, ::4, ::5] = 0.0                                                   # points at infinity
    w = rng.uniform(0.1, 2, (B, H, W)).astype(np.float32)
    mask = (rng.random((B, H, W)) < 0.05).astype(np.uint8)
    R = np.stack([ec.ROTATIONS[(b + seed) % 3][1](W) for b in range(B)]).astype(np.float32)
    T = np.stack([0.3 * pr.unit(pc.TRANSLATIONS[(b + seed) % 3]) for b in range(B)]).astype(np.float32)
    return d, w, mask, R, T


def check_project(got, d, w, mask, R, T, what):
    """The emulation's / device's projection against float64 under the derived bound -> worst error / bound."""
    flow, dn, valid = got
    rf, rd, rv, S, L = rr.project(d, w, R, T, mask)
    du, dv, rel = rr.project_bound(d, T, S, L)
    W = d.shape[2]
    assert (valid == rv).all(), what
    k = rv != 0
    eu, ev = np.abs(rr.wrap_diff(flow[:, 0], rf[:, 0], W)), np.abs(flow[:, 1] - rf[:, 1])
    ed = np.abs(dn - rd)
    worst = max(float((eu[k] / du[k]).max()), float((ev[k] / dv[k]).max()), float((ed[k] / (rel[k] * rd[k] + 1e-45)).max()))
    assert worst <= 1.0, (what, worst)
    assert (flow[:, 0][~k] == 0).all() and (flow[:, 1][~k] == 0).all() and (dn[~k] == 0).all(), what
    return worst


@pytest.mark.parametrize("B,H,W", ((1, 6, 10), (2, 17, 37), (3, 24, 48), (1, 33, 70), (2, 64, 128), (2, 40, 1100)))
def test_project_against_float64(emu, B, H, W):
    d, w, mask, R, T = project_inputs(B, H, W, H)
    d[0, 0, :4] = [np.nan, np.inf, -1.0, 2.0 ** 30]
    w[0, 1, :3] = [0.0, -1.0, np.nan]
    worst = check_project(rc.project_run(emu, d, w, R, T, mask), d, w, mask, R, T, f"{B}x{H}x{W}")
    print(f"[reproject] project {B}x{H}x{W}: worst error / bound {worst:.3f}")
    flow, dn, valid = rc.project_run(emu, d, w, R, T, mask)
    assert valid[0, 0, :4].sum() == 0 and valid[0, 1, :3].sum() == 0 and (valid[mask != 0] == 0).all()
    assert (dn[:, ::4, ::5] == 0).all() and valid[:, ::4, ::5].sum() > 0, "a point at infinity is legal and stays at infinity"


@pytest.mark.parametrize("H,W", rc.TRUTH_SHAPES)
def test_rigid_flow_is_scene_flow(emu, H, W):
    """rigid_flow of the TRUE depth and pose is epipolar_ref.scene_flow, on both depth fields and three poses."""
    from prior_flow_amd.reproject import rigid_flow
    worst = 0.0
    for depth in ("smooth", "room"):
        rho = pr.DEPTHS[depth](H, W)
        for i in range(3):
            R, t, Tn = ec.ROTATIONS[i][1](W), pr.unit(pc.TRANSLATIONS[i]), 0.1 * (i + 1)
            truth = pr.scene_flow(R.astype(np.float32), t, Tn, rho)
            d = (1.0 / rho).astype(np.float32)[None]
            w = np.ones_like(d)
            R32, T32 = R.astype(np.float32)[None], (Tn * t).astype(np.float32)[None]
            ref = rr.project(d, w, R32, T32)
            du, dv, _ = rr.project_bound(d, T32, ref[3], ref[4])
            # the float64 restatement against the generator: only the fp32 roundings of the INPUTS (d, T) separate them
            slack = 8 * U * W * (1 + np.abs(truth).max())
            assert np.abs(rr.wrap_diff(ref[0][0, 0], truth[0], W)).max() <= slack and np.abs(ref[0][0, 1] - truth[1]).max() <= slack
            flow = rigid_flow(*(torch.from_numpy(x) for x in (d, w, R32, T32)), lib=emu)[0].numpy()
            eu, ev = np.abs(rr.wrap_diff(flow[0, 0], truth[0], W)), np.abs(flow[0, 1] - truth[1])
            worst = max(worst, float((eu / (du[0] + slack)).max()), float((ev / (dv[0] + slack)).max()))
    print(f"[reproject] rigid flow against scene_flow {H}x{W}: worst error / bound {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("H,W", ((6, 10), (33, 70), (24, 48)))
def test_project_exact_properties(emu, H, W):
    d, w, mask, R, _ = project_inputs(2, H, W, 3)
    Z = np.zeros((2, 3), np.float32)
    flow, dn, valid = rc.project_run(emu, d, w, R, Z, mask)
    k = valid != 0
    assert (bits(dn[k]) == bits(d[k])).all(), "T = 0 changes no depth, bit for bit"
    for b in range(2):                                                      # the rotation's own flow: derotate's geometry, the other way
        want = er.flow_of(R[b].astype(np.float64), H, W)
        _, _, _, S, L = rr.project(d[b:b + 1], w[b:b + 1], R[b:b + 1], Z[b:b + 1], mask[b:b + 1])
        du, dv, _ = rr.project_bound(d[b:b + 1], Z[b:b + 1], S, L)
        kb = k[b]
        assert (np.abs(rr.wrap_diff(flow[b, 0], want[0], W))[kb] <= du[0][kb]).all() and (np.abs(flow[b, 1] - want[1])[kb] <= dv[0][kb]).all()
    back = er.derotate(np.zeros((2, 2, H, W)), np.transpose(R, (0, 2, 1)))[0]
    assert np.abs(rr.wrap_diff(back[:, 0], rr.project(d, w, R, Z)[0][:, 0], W)).max() < 1e-9
    eye = np.stack([np.eye(3, dtype=np.float32)] * 2)
    flow, dn, valid = rc.project_run(emu, d, w, eye, Z, mask)
    assert (flow == 0).all() and (bits(dn[valid != 0]) == bits(d[valid != 0])).all(), "R = I, T = 0: nothing moves"


# ---- z-splat ---------------------------------------------------------------------------------------------------------------------
def family_properties(family, inp, res):
    src, flow, d, weight, valid = inp
    _, _, out, d_out, w_out, hole, _, _ = res
    if family == "two_layers":
        W2 = d.shape[2] // 2                                              # the pairs (even, odd); an odd width leaves one column alone
        assert (hole[:, :, 0:2 * W2:2] == 0).all() and (d_out[:, :, 0:2 * W2:2] == 4).all(), "the near layer alone decides"
        assert (hole[:, :, 1::2] == 1).all()
        if src is not None:
            W2 = d.shape[2] // 2
            for c in range(src.shape[1]):
                assert (out[:, c, :, 0:2 * W2:2] == c + 10).all(), "the payload is the near layer's"
    if family == "blend":
        W2 = d.shape[2] // 2
        mid = d_out[:, :, 0:2 * W2:2]
        assert ((mid > 1) & (mid < 1.125)).all(), "layers inside the tolerance blend"
    if family == "passthrough":
        with np.errstate(invalid="ignore"):
            counts = weight > 0
            if src is not None:
                counts &= (np.abs(src) < 2.0 ** 30).all(1)
        assert ((hole == 0) == counts).all()
        # the product w_n d is rounded once (U) and quantised to 2^-S_N, the quotient is rounded once more
        sn = rr.scales(d.shape[1], d.shape[2], 65536.0)[1]
        wn = np.minimum(weight, 8.0) / 8.0
        bound = 3 * U + 2.0 ** -sn / (wn[counts] * d[counts])
        assert (np.abs(d_out[counts].astype(np.float64) / d[counts] - 1) <= bound).all()


@pytest.mark.parametrize("B,C,H,W", rc.SWEEP)
@pytest.mark.parametrize("family", rc.FAMILIES)
def test_zsplat_bit_for_bit(emu, family, B, C, H, W):
    """Emulation against the fp32 restatement: front, raw sums, outputs, hole bytes; the buffers all-zero afterwards; outputs
    pre-filled with NaN / 255 fully overwritten."""
    inp = rc.staged(family, B, C, H, W)
    got, ref = rc.zsplat_run(emu, *inp), rr.zsplat(*inp)
    rc.same_bits(got, ref, f"{family} {B}x{C}x{H}x{W}")
    assert not got[6].any() and not got[7].any(), "front and the sums are all-zero after a call"
    for x in got[2:5]:
        assert x is None or np.isfinite(x).all()
    assert set(np.unique(got[5])) <= {0, 1}
    if family != "junk":
        assert (got[5] == 0).any()
    family_properties(family, inp, got)
    if family == "junk":
        rc.same_bits(got, rc.zsplat_run(emu, *rc.junk_as_invalid(*inp)), "junk as invalid")
    if family == "passthrough":                                             # front = 0 admits everything: no z-test, the same bits
        rc.same_bits(got[1:], rr.zsplat(*inp, fault="no_ztest")[1:], "passthrough without a test")


@pytest.mark.parametrize("B,C,H,W", ((2, 3, 24, 48), (2, 1, 17, 37)))
def test_zsplat_order_and_element_form(emu, B, C, H, W):
    inp = rc.staged("collapse", B, C, H, W)[:1] + rc.staged("seam", B, C, H, W)[1:]
    base = rc.zsplat_run(emu, *inp)
    try:
        for seed in (1, 12345):
            emu._dll.pf_emu_odo_order(seed)
            rc.same_bits(rc.zsplat_run(emu, *inp), base, f"order {seed}")
    finally:
        emu._dll.pf_emu_odo_order(0)
    rc.same_bits(rc.zsplat_run(emu, *inp, offset=1), base, "unaligned maps: the element form")
    # which form those two calls took, from the rule the entry points apply themselves
    emu._dll.pf_emu_zsplat_quads.argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_int]
    forms = []
    for offset in (0, 1):
        z = rc.ZRun(emu, B, C, H, W, offset=offset)
        forms.append(emu._dll.pf_emu_zsplat_quads(*(x.data_ptr() for x in (z.acc, z.front, z.out, z.d_out, z.w_out, z.hole)), W))
    assert forms == [1 if W % 4 == 0 else 0, 0]


# ---- truth -----------------------------------------------------------------------------------------------------------------------
TRUTH_REF = {}


def truth_run(lib, pair, device="cpu", fault=None):
    """(restatement's tuple, lib's tuple or None, the later frame's true inverse depth, the pair's third element)."""
    d0, d1, extra, R, T = pair
    d0 = d0.astype(np.float32)[None]
    w = np.ones_like(d0)
    ref = rr.reproject(None, d0, w, R, T, fault=fault)
    got = None
    if lib is not None:
        flow, dn, valid = rc.project_run(lib, d0, w, R, T, None, device)
        got = rc.zsplat_run(lib, None, flow, dn, w, valid, device)
    return ref, got, d1, extra


def convex_cap(H, W):
    """Twice the restatement's worst relative error on the convex scene of that size (section 22's convention)."""
    ref, _, d1, _ = truth_run(None, rc.pair(rc.CONVEX, 0, H, W))
    return 2 * rc.rel_error(ref[3][0], ref[5][0], d1)[0]


@pytest.mark.parametrize("H,W", rc.TRUTH_SHAPES)
def test_convex_scene_against_truth(emu, H, W):
    ref, got, d1, _ = truth_run(emu, rc.pair(rc.CONVEX, 0, H, W))
    e_ref, h_ref = rc.rel_error(ref[3][0], ref[5][0], d1)
    e_got, h_got = rc.rel_error(got[3][0], got[5][0], d1)
    TRUTH_REF[(H, W)] = e_ref
    print(f"[reproject] convex {H}x{W}: restatement worst relative error {e_ref:.3e}, holes {h_ref:.2%}; emulation {e_got:.3e}, {h_got:.2%}")
    assert h_ref <= rc.HOLE_CAP and h_got <= rc.HOLE_CAP
    assert e_got <= 2 * e_ref


def occluder_check(lib, H, W, device="cpu"):
    """The occluder scene at one size through `lib` -> (restatement's, lib's, the no-z-test twin's worst error / bound)."""
    cap = convex_cap(H, W)
    pair = rc.occluder_pair(H, W)
    ref, got, d1, info = truth_run(lib, pair, device)
    wrong = truth_run(None, pair, fault="no_ztest")[0]
    e_ref, u_ref, n_ref = rc.occluder_error(ref[3][0], ref[5][0], d1, info, cap)
    e_got, u_got, _ = rc.occluder_error(got[3][0], got[5][0], d1, info, cap)
    e_bad = rc.occluder_error(wrong[3][0], wrong[5][0], d1, info, cap)[0]
    k = info["reached"] & (ref[5][0] == 0)
    rel = np.abs(ref[3][0] / d1 - 1)
    print(f"[reproject] occluder {H}x{W}: silhouette {int(info['region'].sum())} px, judged {n_ref}, not judged {u_ref:.1%} (cap "
          f"{rc.occluder_unjudged_cap(H, W):.1%}); worst error / bound restatement {e_ref:.3f}, {'device' if device != 'cpu' else 'emulation'} "
          f"{e_got:.3f}, without the z-test {e_bad:.3f}; plain relative error: worst {rel[k].max():.3e}, median {np.median(rel[k]):.3e}, "
          f"{int((rel[k] <= cap).sum())} of {n_ref} within the convex cap {cap:.3e}")
    assert n_ref >= 8
    assert u_ref <= rc.occluder_unjudged_cap(H, W) and u_got <= rc.occluder_unjudged_cap(H, W)
    return e_ref, e_got, e_bad


@pytest.mark.parametrize("H,W", rc.OCCLUDER_SHAPES)
def test_occluder_scene(emu, H, W):
    """On the WHOLE new silhouette of the ball the output is the ball's depth: within the convex scene's cap of that size plus the
    spread of the ball's own inverse depth over the taps' reach (reproject_cases.occluder_pair derives it per pixel; the ball's
    depth changes by tens of per cent within a pixel towards its limb, so the plain cap cannot hold there for any splat of a
    sampled map).  Without the z-test it is not, at every size: the background seen in the earlier frame lands there too."""
    e_ref, e_got, e_bad = occluder_check(emu, H, W)
    assert e_ref <= 1 and e_got <= 1
    assert e_bad > 1, "the seeded fault no_ztest passed"


# ---- update ----------------------------------------------------------------------------------------------------------------------
def check_update(got, ds, ws, dm, wm, dis, flags, seg, what):
    """Against float64 within UPDATE_U per element; where a log2 near tol decides, either branch is accepted -> (count of
    elements that differ from the fp32 restatement, worst error / bound)."""
    d, w, sg = got
    r64 = rr.update(ds, ws, dm, wm, dis, flags, seg)
    r32 = rr.update(ds, ws, dm, wm, dis, flags, seg, np.float32)
    assert (sg == r64[2]).all(), what
    edge = r64[3] & rr.near_tol(ds, dm, rr.DEFAULTS["tol_log2"])
    bd = rr.UPDATE_U * np.abs(r64[0]) + 1e-45
    bw = rr.UPDATE_U * np.abs(r64[1]) + 1e-45
    err = np.maximum(np.abs(d - r64[0]) / bd, np.abs(w - r64[1]) / bw)
    assert np.isfinite(d).all() and np.isfinite(w).all(), what
    assert (err[~edge] <= 1).all(), (what, float(err[~edge].max()))
    differ = int(((bits(d) != bits(r32[0])) | (bits(w) != bits(r32[1])))[~edge].sum())
    return differ, float(err[~edge].max()), int(edge.sum())


@pytest.mark.parametrize("B,H,W", ((1, 6, 10), (2, 17, 37), (3, 24, 48)))
def test_update_against_float64(emu, B, H, W):
    ds, ws, dm, wm, dis = rc.update_inputs(B, H, W, H)
    flags = np.array([[3, 2, 1, 1]] * B, np.int32)
    seg = np.full(B, 2, np.int32)
    got = rc.update_run(emu, ds, ws, dm, wm, dis, flags, seg)
    differ, worst, edge = check_update(got, ds, ws, dm, wm, dis, flags, seg, f"update {B}x{H}x{W}")
    print(f"[reproject] update {B}x{H}x{W}: worst error / bound {worst:.3f}; {differ} values differ from the fp32 restatement, {edge} at the edge of tol")
    assert differ == 0
    if (H * W) % 4 == 0:
        unaligned = rc.update_run(emu, ds, ws, dm, wm, dis, flags, seg, offset=1)
        assert all((bits(a) == bits(b)).all() for a, b in zip(got, unaligned)), "the element form gives the quad form's bits"


def update_rules(lib, device="cpu"):
    """The rules of the update one by one, on constant maps."""
    B, H, W = 2, 4, 8
    run = lambda *a: rc.update_run(lib, *a, device=device)                # noqa: E731
    one = lambda v: np.full((B, H, W), v, np.float32)                     # noqa: E731
    flags, seg = np.array([[5, 3, 1, 1], [5, 3, 1, 1]], np.int32), np.array([3, 2], np.int32)
    # a segment change zeroes the old state of THAT image only, and seg follows
    d, w, sg = run(one(2), one(4), one(2), one(1), None, flags, seg)
    assert (w[0] == np.float32(0.9) * 4 + 1).all() and (w[1] == 1).all() and (sg == [3, 3]).all()
    seg = np.array([3, 3], np.int32)
    # disagree and invalid measurements are ignored: the state stays, decayed
    dis = np.ones((B, H, W), np.uint8)
    d, w, _ = run(one(2), one(4), one(3), one(1), dis, flags, seg)
    assert (d == 2).all() and (w == np.float32(0.9) * 4).all()
    for bad in (np.nan, -1.0, 2.0 ** 30, np.inf):
        d, w, _ = run(one(2), one(4), one(bad), one(1), None, flags, seg)
        assert (d == 2).all() and (w == np.float32(0.9) * 4).all(), bad
    # beyond tol the measurement replaces the state
    d, w, _ = run(one(2), one(4), one(3), one(1), None, flags, seg)
    assert (d == 3).all() and (w == 1).all()
    # inside tol: the weighted mean, the weight saturating at w_max
    d, w, _ = run(one(2), one(8), one(2.5), one(4), None, flags, seg)
    assert (w == 8).all() and ((d > 2) & (d < 2.5)).all()
    # neither counts: 0, 0, never NaN
    d, w, _ = run(one(np.nan), one(0), one(0), one(0), None, flags, seg)
    assert (d == 0).all() and (w == 0).all()
    d, w, _ = run(one(0), one(1), one(0), one(1), None, flags, seg)     # two points at infinity: log2(0 / 0)
    assert (d == 0).all() and np.isfinite(w).all()
    d, w, _ = run(one(1e9), one(3e38), one(1e9), one(3e38), None, flags, seg)
    assert np.isfinite(d).all() and (w == 8).all()


def test_update_rules(emu):
    update_rules(emu)


FILTER_REF = {}


def test_filter_has_a_point(emu):
    H, W = 32, 64
    ratios = []
    for seed in (0, 1, 2):
        f, s = rc.filter_path(*rc.ref_filter(), H, W, seed)
        ratios.append(f / s)
    f, s = rc.filter_path(*rc.lib_filter(emu), H, W, 0)
    spread = max(ratios) / min(ratios)
    FILTER_REF["ratio"], FILTER_REF["spread"] = ratios[0], spread
    print(f"[reproject] filter {H}x{W}: restatement rms log2 error filtered / single = {ratios[0]:.3f} (seeds 1, 2: {ratios[1]:.3f}, {ratios[2]:.3f}; "
          f"spread {spread:.3f}); emulation {f / s:.3f}")
    assert all(r < 1 for r in ratios) and f < s
    assert spread <= rc.FILTER_FACTOR, "the factor must cover the restatement's own spread"
    assert f / s <= ratios[0] * rc.FILTER_FACTOR


# ---- seeded faults ---------------------------------------------------------------------------------------------------------------
def test_every_seeded_fault_is_caught(emu):
    caught = {}
    H, W = 32, 64
    # the projection's faults: the truth of the convex scene (test_convex_scene_against_truth's check)
    d0, d1, _, R, T = rc.pair(rc.CONVEX, 0, H, W)
    d0 = d0.astype(np.float32)[None]
    one = np.ones_like(d0)
    good = rr.reproject(None, d0, one, R, T)
    cap = 2 * rc.rel_error(good[3][0], good[5][0], d1)[0]
    for fault in ("d_not_divided", "t_sign"):
        bad = rr.reproject(None, d0, one, R, T, fault=fault)
        caught[fault] = rc.rel_error(bad[3][0], bad[5][0], d1)[0] > cap
    # a rotation of two degrees inside a sphere barely changes a depth: the flow shows it (test_project_against_float64's check)
    twin = rr.project(d0, one, R, T, fault="r_transposed")
    du, _, _ = rr.project_bound(d0, T, twin[3], twin[4])
    caught["r_transposed"] = bool((np.abs(rr.wrap_diff(rc.project_run(emu, d0, one, R, T)[0][:, 0], twin[0][:, 0], W)) > du).any())
    # the splat's faults: the bits of the emulation on the sweep's families (test_zsplat_bit_for_bit's check)
    def differs(fault, family, part=slice(0, 8)):
        inp = rc.staged(family, 2, 3, 24, 48)
        got, twin = rc.zsplat_run(emu, *inp), rr.zsplat(*inp, fault=fault)
        try:
            rc.same_bits(got[part], twin[part], fault)
        except AssertionError:
            return True
        return False
    o_pair = rc.occluder_pair(32, 64)
    wrong = truth_run(None, o_pair, fault="no_ztest")[0]
    caught["no_ztest"] = rc.occluder_error(wrong[3][0], wrong[5][0], o_pair[1], o_pair[2], convex_cap(32, 64))[0] > 1 \
        and differs("no_ztest", "two_layers")
    caught["ztest_min"] = differs("ztest_min", "two_layers")
    caught["bmin_ignored"] = differs("bmin_ignored", "seam")
    caught["front_not_cleared"] = differs("front_not_cleared", "seam", slice(6, 7))
    caught["weights_not_normalised"] = differs("weights_not_normalised", "seam")
    # the update's faults: test_update_rules' and test_update_against_float64's checks
    ds, ws, dm, wm, dis = rc.update_inputs(2, 8, 16, 5)
    flags, seg = np.array([[3, 2, 1, 1], [3, 2, 1, 1]], np.int32), np.array([2, 1], np.int32)
    got = rc.update_run(emu, ds, ws, dm, wm, dis, flags, seg)
    for fault in ("segment_ignored", "decay_dropped"):
        twin = rr.update(ds, ws, dm, wm, dis, flags, seg, np.float32, fault)
        caught[fault] = bool((bits(twin[0]) != bits(got[0])).any() or (bits(twin[1]) != bits(got[1])).any())
    assert set(caught) == set(rr.FAULTS)
    assert all(caught.values()), [k for k, v in caught.items() if not v]


# ---- the Python layer ------------------------------------------------------------------------------------------------------------
def test_reprojector_and_propagator_are_their_entry_points(emu):
    from prior_flow_amd.odometry import Odometry
    from prior_flow_amd.reproject import DepthPropagator, Reprojector, reproject
    B, C, H, W = 2, 3, 24, 48
    d, w, mask, R, T = project_inputs(B, H, W, 1)
    src = np.random.default_rng(0).uniform(0, 255, (B, C, H, W)).astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))               # noqa: E731
    flow, dn, valid = rc.project_run(emu, d, w, R, T, mask)
    want = rc.zsplat_run(emu, src, flow, dn, w, valid)
    rp = Reprojector(B, C, H, W, "cpu", lib=emu)
    for _ in range(2):                                                      # the second run starts from what the first left
        out = rp.run(t(src), t(d), t(w), t(R), t(T), t(mask))
        for a, b in zip(out, want[2:6]):
            assert (bits(a.numpy()) == bits(b)).all()
    once = reproject(t(src), t(d), t(w), t(R), t(T), t(mask), lib=emu)
    assert all((bits(a.numpy()) == bits(b)).all() for a, b in zip(once, want[2:6]))
    # a propagator behind an Odometry whose outputs are set by hand (its own push is section 22's)
    odo = Odometry(B, H, W, "cpu", lib=emu)
    prop = DepthPropagator(odo, channels=C)
    odo.pose.R.copy_(t(R))
    odo.pose.t.copy_(t(T / 0.3))
    odo.baseline.fill_(0.3)
    odo.flags.copy_(torch.tensor([[1, 1, 1, 0]] * B, dtype=torch.int32))
    odo.map_b[3].copy_(t(mask))
    ds, ws = np.zeros((B, H, W), np.float32), np.zeros((B, H, W), np.float32)
    seg = np.zeros(B, np.int32)
    for step in range(3):
        dm, wm, _, _, _ = project_inputs(B, H, W, 10 + step)
        dis = (np.random.default_rng(step).random((B, H, W)) < 0.1).astype(np.uint8)
        odo.inv_depth.copy_(t(dm)); odo.depth_weight.copy_(t(wm)); odo.disagree.copy_(t(dis))
        fd, fw = prop.push(frame=t(src))
        ud, uw, seg = rc.update_run(emu, ds, ws, dm, wm, dis, odo.flags.numpy(), seg)
        assert (bits(fd.numpy()) == bits(ud)).all() and (bits(fw.numpy()) == bits(uw)).all(), step
        Tn = (odo.baseline[:, None] * odo.pose.t).numpy()
        flow, dn, valid = rc.project_run(emu, ud, uw, R, Tn, mask)
        z = rc.zsplat_run(emu, src, flow, dn, uw, valid)
        assert (bits(prop.rigid_flow.numpy()) == bits(flow)).all()
        for a, b in zip((prop.predicted_frame, prop.predicted_inv_depth, prop.predicted_weight, prop.hole), z[2:6]):
            assert (bits(a.numpy()) == bits(b)).all(), step
        ds, ws = z[3], z[4]
    # reset: poisoned state gives a fresh object's bits
    for x in (prop.inv_depth, prop.weight, prop.rp.inv_depth, prop.rp.weight, prop.rp.flow, prop.rp.d_new):
        x.fill_(float("nan"))
    prop.rp.acc.fill_(1 << 40); prop.rp.front.fill_(0x7F000000); prop.seg.fill_(9)
    prop.reset()
    fresh = DepthPropagator(odo, channels=C)
    a, b = prop.push(frame=t(src)), fresh.push(frame=t(src))
    assert all((bits(x.numpy()) == bits(y.numpy())).all() for x, y in zip(a, b))
    assert (bits(prop.predicted_inv_depth.numpy()) == bits(fresh.predicted_inv_depth.numpy())).all()


def test_python_refusals_launch_nothing(emu):
    from prior_flow_amd._lib import PfError
    from prior_flow_amd.reproject import DepthPropagator, Reprojector, reproject, rigid_flow
    B, C, H, W = 1, 1, 6, 10
    d, w, mask, R, T = (torch.from_numpy(x) for x in project_inputs(B, H, W, 0))
    src = torch.zeros(B, C, H, W)
    rp = Reprojector(B, C, H, W, "cpu", lib=emu)
    bad = [lambda: rp.run(src, d.double(), w, R, T), lambda: rp.run(src, d, w[:, :, :5], R, T), lambda: rp.run(None, d, w, R, T),
           lambda: rp.run(src, d.transpose(1, 2).contiguous().transpose(1, 2), w, R, T), lambda: rp.run(src, d, w, R, T, mask.float()),
           lambda: rp.run(src, rp.inv_depth, w, R, T), lambda: rp.run(src, d, rp.weight, R, T), lambda: rp.run(rp.out, d, w, R, T),
           lambda: rigid_flow(d, w, R, T, out=(torch.zeros(B, 2, H, W), d, torch.zeros(B, H, W, dtype=torch.uint8)), lib=emu),
           lambda: rigid_flow(d, w, R, T, n_min=0.0, lib=emu), lambda: reproject(src[0], d, w, R, T, lib=emu),
           lambda: Reprojector(B, 5, H, W, "cpu", lib=emu), lambda: Reprojector(B, C, H, W, "cpu", lib=emu, b_min=2.0),
           lambda: Reprojector(B, C, H, W, "cpu", lib=emu, nonsense=1), lambda: Reprojector(B, C, H, W, "cpu", lib=emu, b_min="a lot"),
           lambda: Reprojector(B, C, H, W, "cpu", lib=emu, cmin=None), lambda: DepthPropagator(object()),
           lambda: rigid_flow(d, w, R, T), lambda: Reprojector(B, C, H, W, "cpu")]          # host tensors without the emulation's handle
    for i, f in enumerate(bad):
        with pytest.raises(PfError):
            f()
        assert not rp.acc.any() and not rp.front.any(), i


# ---- the C checks ----------------------------------------------------------------------------------------------------------------
def test_every_rule_of_every_check(emu):
    """Each rule of pf_reproj_project_check, pf_zsplat_check, pf_zsplat_resolve_check and pf_depth_update_check once, through the
    raw entry points: a refused call returns its code and leaves every buffer as it was."""
    dll = emu._dll
    B, C, H, W = 1, 1, 4, 8
    N = B * H * W
    buf = np.zeros(8 * N * 16 + 32, np.uint8)
    base = buf.ctypes.data + (-buf.ctypes.data) % 16
    p = lambda k: ctypes.c_void_p(base + k * 8 * N)                        # noqa: E731  disjoint slots, 16-byte aligned
    odd = lambda k: ctypes.c_void_p(base + k * 8 * N + 2)                  # noqa: E731
    Z = None
    ARG, SHAPE = -1, -2

    def project(**kw):
        a = dict(d=p(0), w=p(1), m=p(2), R=p(3), T=p(4), flow=p(5), dn=p(6), v=p(7), B=B, H=H, W=W, n=1e-6)
        a.update(kw)
        return dll.pf_reproj_project(a["d"], a["w"], a["m"], a["R"], a["T"], a["flow"], a["dn"], a["v"], a["B"], a["H"], a["W"], a["n"], None)

    def front(**kw):
        a = dict(s=p(0), f=p(1), d=p(2), w=p(3), v=p(4), fr=p(5), B=B, C=C, H=H, W=W, b=0.25)
        a.update(kw)
        return dll.pf_zsplat_front(a["s"], a["f"], a["d"], a["w"], a["v"], a["fr"], a["B"], a["C"], a["H"], a["W"], a["b"], None)

    def acc(**kw):
        a = dict(s=p(0), f=p(1), d=p(2), w=p(3), v=p(4), fr=p(5), acc=p(8), B=B, C=C, H=H, W=W, b=0.25, tol=0.25, wm=8.0, dm=65536.0, vm=255.0)
        a.update(kw)
        return dll.pf_zsplat_accumulate(a["s"], a["f"], a["d"], a["w"], a["v"], a["fr"], a["acc"], a["B"], a["C"], a["H"], a["W"], a["b"],
                                        a["tol"], a["wm"], a["dm"], a["vm"], None)

    def resolve(**kw):
        a = dict(acc=p(8), fr=p(5), out=p(0), d=p(1), w=p(2), h=p(3), B=B, C=C, H=H, W=W, c=0.5, wm=8.0, dm=65536.0, vm=255.0)
        a.update(kw)
        return dll.pf_zsplat_resolve(a["acc"], a["fr"], a["out"], a["d"], a["w"], a["h"], a["B"], a["C"], a["H"], a["W"], a["c"], a["wm"],
                                     a["dm"], a["vm"], None)

    def update(**kw):
        a = dict(ds=p(0), ws=p(1), dm=p(2), wm=p(3), dis=p(4), fl=p(5), sg=p(6), B=B, H=H, W=W, tol=0.5, dec=0.9, wx=8.0)
        a.update(kw)
        return dll.pf_depth_update(a["ds"], a["ws"], a["dm"], a["wm"], a["dis"], a["fl"], a["sg"], a["B"], a["H"], a["W"], a["tol"], a["dec"],
                                   a["wx"], None)

    nan, inf = float("nan"), float("inf")
    shapes = [dict(B=0), dict(H=0), dict(W=0), dict(B=65536), dict(H=1 << 15, W=1 << 15)]
    rules = []
    rules += [(project, k, ARG) for k in (dict(d=Z), dict(w=Z), dict(R=Z), dict(T=Z), dict(flow=Z), dict(dn=Z), dict(v=Z), dict(d=odd(0)),
                                          dict(w=odd(1)), dict(R=odd(3)), dict(T=odd(4)), dict(flow=odd(5)), dict(dn=odd(6)), dict(n=0.0),
                                          dict(n=nan), dict(n=inf), dict(flow=p(0)), dict(dn=p(1)), dict(v=p(2)), dict(dn=p(5)), dict(v=p(6)),
                                          dict(flow=p(3)), dict(dn=p(4)))]
    rules += [(project, k, SHAPE) for k in shapes]
    for fn in (front, acc):
        rules += [(fn, k, ARG) for k in (dict(f=Z), dict(d=Z), dict(w=Z), dict(v=Z), dict(fr=Z), dict(s=Z), dict(C=0), dict(C=5), dict(C=-1),
                                         dict(s=odd(0)), dict(f=odd(1)), dict(d=odd(2)), dict(w=odd(3)), dict(fr=odd(5)), dict(b=-0.1),
                                         dict(b=1.5), dict(b=nan), dict(fr=p(1)), dict(fr=p(0)), dict(fr=p(2)), dict(fr=p(3)), dict(fr=p(4)))]
        rules += [(fn, k, SHAPE) for k in shapes]
    rules += [(acc, k, ARG) for k in (dict(acc=Z), dict(acc=ctypes.c_void_p(base + 64 * N + 4)), dict(tol=-1.0), dict(tol=65.0), dict(tol=nan),
                                      dict(wm=0.0), dict(wm=inf), dict(dm=0.5), dict(dm=1e6), dict(vm=0.5), dict(vm=1e6), dict(acc=p(1)),
                                      dict(acc=p(5)), dict(acc=p(0)))]
    rules += [(resolve, k, ARG) for k in (dict(acc=Z), dict(fr=Z), dict(d=Z), dict(w=Z), dict(h=Z), dict(out=Z), dict(C=0), dict(C=5),
                                          dict(acc=ctypes.c_void_p(base + 64 * N + 4)), dict(fr=odd(5)), dict(out=odd(0)), dict(d=odd(1)),
                                          dict(w=odd(2)), dict(c=0.0), dict(c=nan), dict(wm=0.0), dict(wm=nan), dict(dm=0.5), dict(vm=1e6),
                                          dict(fr=p(8)), dict(out=p(8)), dict(d=p(0)), dict(w=p(1)), dict(h=p(2)), dict(h=p(5)))]
    rules += [(resolve, k, SHAPE) for k in shapes]
    rules += [(update, k, ARG) for k in (dict(ds=Z), dict(ws=Z), dict(dm=Z), dict(wm=Z), dict(fl=Z), dict(sg=Z), dict(ds=odd(0)), dict(ws=odd(1)),
                                         dict(dm=odd(2)), dict(wm=odd(3)), dict(fl=odd(5)), dict(sg=odd(6)), dict(tol=0.0), dict(tol=nan),
                                         dict(dec=0.0), dict(dec=1.5), dict(dec=nan), dict(wx=0.0), dict(wx=inf), dict(ds=p(2)), dict(ws=p(3)),
                                         dict(ds=p(1)), dict(sg=p(5)), dict(ws=p(4)), dict(sg=p(0)))]
    rules += [(update, k, SHAPE) for k in shapes]
    for fn, kw, want in rules:
        assert fn(**kw) == want, (fn.__name__, kw)
        assert not buf.any(), (fn.__name__, kw, "a refused call wrote")
    # the same calls without a fault are accepted (all-zero inputs: nothing counts), optional pointers may be NULL
    assert project() == 0 and project(m=Z) == 0 and front() == 0 and acc() == 0 and resolve() == 0 and update() == 0 and update(dis=Z) == 0
    assert front(s=Z, C=0) == 0 and acc(s=Z, C=0) == 0 and resolve(out=Z, C=0) == 0
    assert emu.zsplat_bytes(2, 3, 4, 8) == 2 * 6 * 32 * 8 and dll.pf_zsplat_bytes(1, 5, 4, 8) == ARG and dll.pf_zsplat_bytes(0, 1, 4, 8) == SHAPE
