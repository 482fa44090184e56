"""Perspective viewports and cube maps without a GPU: the float64 statement (tests/viewport_ref.py), the host
emulation of pf_viewport_image / pf_viewport_flow / pf_cubemap_to_erp (tests/emu/pf_emu_viewport.cpp over csrc/pf_viewport.h, the
header the device kernels compile) under the derived per-pixel bounds of tests/viewport_cases.py, the seeded faults, and the
refusals of the built library.

Measured on the emulation (x86-64, glibc): the largest |err| / bound over all cases is 0.126 for fp32 images, 0.029 for the flow and
0.075 for cube maps; one byte of all uint8 views differs from the float64 statement's rounded value (by 1, at a value within the
bound of a half-integer; 0.2 - 0.7 % of a case's values lie that near).  No cosine of a case lies within 1e-5 of min_forward.
"""
import ctypes
import shutil

import numpy as np
import pytest

import viewport_cases as vc
import viewport_ref as vr


@pytest.fixture(scope="module")
def emu():
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    import __graft_entry__ as ge
    from prior_flow_amd import _lib
    so = ge.build_emu_viewport()
    keep = ("pf_viewport_image", "pf_viewport_flow", "pf_cubemap_to_erp")
    return _lib.PfLib(so, require_cuda=False, optional=tuple(n for n in _lib.EXPORTS if n not in keep))


# ---- geometry facts of the statement -----------------------------------------------------------------------------------------
def test_identity_view_looks_at_the_centre_right_is_m_down_is_n():
    row = vr.viewport_row(0.0, 0.0, 0.0, 90.0, 5, 7)
    m, n = vr.erp_of(vr.rays(row), 32, 64)
    assert abs(m[2, 3] - 31.5) < 1e-12 and abs(n[2, 3] - 15.5) < 1e-12            # the centre of a 32 x 64 map
    assert m[2, 4] > m[2, 3] and abs(n[2, 4] - n[2, 3]) < 1e-12                    # right: +m
    assert n[3, 3] > n[2, 3] and abs(m[3, 3] - m[2, 3]) < 1e-12                    # down: +n
    x, y, _ = vr.proj(vr.rays(row), row)                                           # proj inverts the rays
    j, i = np.meshgrid(np.arange(7.0), np.arange(5.0))
    assert np.abs(x - j).max() < 1e-12 and np.abs(y - i).max() < 1e-12
    # the sphere map and its inverse
    mm, nn = np.meshgrid(np.arange(64.0), np.arange(32.0))
    m2, n2 = vr.erp_of(vr.sphere(mm, nn, 32, 64), 32, 64)
    assert np.abs(m2 - mm).max() < 1e-9 and np.abs(n2 - nn).max() < 1e-9
    # a positive pitch looks down (the sign that Rz Ry Rx gives), a positive yaw to the right
    md, nd = vr.erp_of(vr.rays(vr.viewport_row(0.0, 0.3, 0.0, 90.0, 5, 7)), 32, 64)
    assert nd[2, 3] > 15.5 and abs(md[2, 3] - 31.5) < 1e-9
    my, _ = vr.erp_of(vr.rays(vr.viewport_row(0.3, 0.0, 0.0, 90.0, 5, 7)), 32, 64)
    assert my[2, 3] > 31.5


def test_python_views_are_the_statements():
    from prior_flow_amd import projection as pj
    for y, p, r, fov in vc.VIEW_SETS[7]:
        assert np.allclose(pj.Viewport(y, p, r, fov, 17, 23).row(), vr.viewport_row(y, p, r, fov, 17, 23), rtol=0, atol=1e-12)
    assert np.array_equal(np.array([v.row() for v in pj.cube_faces(12)]), vr.cube_rows(12))
    assert abs(pj.MIN_FORWARD - vc.MIN_FORWARD) < 1e-15


def test_cube_faces_are_rotations_and_tile_the_sphere():
    for s in vc.CUBE_SIZES:
        rows = vr.cube_rows(s)
        for r in rows:
            R = r[:9].reshape(3, 3)
            assert np.array_equal(R @ R.T, np.eye(3)) and np.linalg.det(R) == pytest.approx(1.0, abs=1e-15)
        face, px, py = vr.cube_positions(s, 32, 64)
        n, m = np.meshgrid(np.arange(32.0), np.arange(64.0), indexing="ij")
        d = vr.sphere(m, n, 32, 64)
        forward = np.stack([d @ r[:9].reshape(3, 3)[:, 0] for r in rows], -1)
        assert (np.isclose(forward, forward.max(-1, keepdims=True), rtol=0, atol=0).sum(-1) == 1).all()   # exactly one face
        assert set(np.unique(face)) == set(range(6))
        assert px.min() >= -0.5 and px.max() <= s - 0.5 and py.min() >= -0.5 and py.max() <= s - 0.5


def test_face_ties_go_to_the_earlier_face(emu):
    want = [0, 0, 1, 0, 1, 2, 0, 2, 3, 2, 0]
    assert vr.cube_face(np.array(vc.TIES)).tolist() == want
    assert vc.emu_faces(emu, vc.TIES).tolist() == want


# ---- exact zero and second-order accuracy ------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", vc.PANORAMAS)
def test_zero_flow_gives_exactly_zero_and_every_valid_bit(emu, H, W):
    for h, w in vc.VIEW_SIZES:
        for V in vc.VIEW_SETS:
            _, t32 = vc.rows_of(V, h, w)
            got, valid = vc.run_flow(emu, vc.make_flow("zero", 2, H, W), t32)
            assert not got.any() and (valid == 1).all(), (H, W, h, w, V)
            want, wvalid, _ = vr.view_flow(vc.make_flow("zero", 1, H, W), t32, vc.MIN_FORWARD)
            assert not want.any() and (wvalid == 1).all()


def test_constant_u_flow_converges_to_the_yaw_rotation_at_second_order(emu):
    """A constant u is the rigid yaw by alpha = 2 pi u / W.  With alpha fixed, halving the pixel pitch must cut the difference
    from the closed form to a quarter (3.1e-2 px at 32x64, 7.7e-3 at 64x128 in the float64 model); the bar is 0.3, the margin
    covering the maximum over four views.  The four views keep clear of the caps within half a row of a pole: there the taps'
    y clamp makes the two rows equal, and the map is first-order in n like every clamped bilinear sampler."""
    t32 = vr.table32([vr.viewport_row(*v, 17, 23) for v in vc.OFF_POLE_VIEWS])
    alpha = 2 * np.pi * 3 / 64
    closed = vr.yaw_flow_closed_form(t32, alpha)
    errs = {}
    for who in ("statement", "emulation"):
        for H, W in ((32, 64), (64, 128)):
            flow = np.zeros((1, 2, H, W), np.float32)
            flow[:, 0] = 3.0 * W / 64
            if who == "statement":
                got, valid, _ = vr.view_flow(flow, t32, vc.MIN_FORWARD)
            else:
                got, valid = vc.run_flow(emu, flow, t32)
            assert (valid == 1).all()
            errs[who, W] = np.abs(got[0] - closed).max()
        print(f"[viewport] constant u against the closed-form yaw, {who}: {errs[who, 64]:.3e} px at 32x64, {errs[who, 128]:.3e} at 64x128, "
              f"ratio {errs[who, 128] / errs[who, 64]:.3f}")
        assert errs[who, 128] <= 0.3 * errs[who, 64]
        assert errs[who, 64] < 0.1


# ---- the emulation against the statement on every case -----------------------------------------------------------------------
@pytest.mark.parametrize("h,w", vc.VIEW_SIZES)
@pytest.mark.parametrize("H,W", vc.PANORAMAS)
def test_emulated_images_hold_the_bounds(emu, H, W, h, w):
    worst = 0.0
    for V in vc.VIEW_SETS:
        for B, C, form in vc.IMAGE_FORMS:
            _, r = vc.image_case(emu, H, W, h, w, V, B, C, form)
            worst = max(worst, r if form == "f32" else 0.0)
    print(f"[viewport] emulated images {H}x{W} -> {h}x{w}: worst ratio {worst:.3f}")


@pytest.mark.parametrize("h,w", vc.VIEW_SIZES)
@pytest.mark.parametrize("H,W", vc.PANORAMAS)
def test_emulated_flows_hold_the_bounds(emu, H, W, h, w):
    worst = max(vc.flow_case(emu, H, W, h, w, V, kind)[2] for V in vc.VIEW_SETS for kind in vc.FLOW_KINDS)
    print(f"[viewport] emulated flows {H}x{W} -> {h}x{w}: worst ratio {worst:.3f}")


def test_smooth_field_leaves_the_views_and_stays_off_the_threshold():
    """The smooth field's end points cross both poles and a share of them lands behind the camera; none of the statement's cosines
    lies within 1e-5 of min_forward in more than 0.5 % of a case (check_flow asserts it case by case; here over all of them)."""
    shares, behind = [], []
    for H, W in vc.PANORAMAS:
        flow = vc.make_flow("smooth", 2, H, W, seed=7)
        n = np.arange(H)[None, :, None] + flow[:, 1]
        assert (n < -0.5).any() and (n > H - 0.5).any()
        for h, w in vc.VIEW_SIZES:
            _, t32 = vc.rows_of(7, h, w)
            _, valid, cosine = vr.view_flow(flow, t32, vc.MIN_FORWARD)
            shares.append(float((np.abs(cosine - vc.MIN_FORWARD) <= 1e-5).mean()))
            behind.append(1.0 - float(valid.mean()))
    print(f"[viewport] smooth field: share behind the camera {min(behind):.3f} .. {max(behind):.3f}; within 1e-5 of min_forward {max(shares):.2e}")
    assert max(shares) <= 0.005 and 0.03 <= min(behind) and max(behind) <= 0.3


@pytest.mark.parametrize("s", vc.CUBE_SIZES)
def test_emulated_cube_maps_hold_the_bounds(emu, s):
    for B, C in ((1, 1), (2, 3)):
        vc.cube_case(emu, s, 32, 64, B, C)
    # ERP -> faces is pf_viewport_image with the six face views
    x = vc.make_image(2, 3, 32, 64, seed=s)
    t32 = vr.table32(vr.cube_rows(s))
    got = vc.run_image(emu, x, t32)
    vc.check_values(got, vr.view_image(x, t32), vc.image_bound(x, t32), f"ERP 32x64 -> cube {s} on cpu")


# ---- seeded faults -----------------------------------------------------------------------------------------------------------
def _breaks(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


@pytest.fixture(scope="module")
def fault_runs(emu):
    """The emulation's outputs on the cases the seeded faults are tried on (computed once)."""
    runs = {"image": [], "flow": [], "cube": []}
    for H, W in vc.PANORAMAS:
        _, t32 = vc.rows_of(7, 17, 23)
        x = vc.make_image(1, 3, H, W, seed=5)
        runs["image"].append((x, vc.run_image(emu, x, t32)))
        for kind in ("u_half", "smooth"):
            flow = vc.make_flow(kind, 1, H, W, seed=3)
            runs["flow"].append((flow, vc.run_flow(emu, flow, t32)))
    for s in vc.CUBE_SIZES:
        faces = vc.make_faces(1, 2, s, seed=s)
        runs["cube"].append((faces, vc.run_cube(emu, faces, 32, 64)))
    return runs


@pytest.mark.parametrize("fault", vr.FAULTS)
def test_a_seeded_fault_breaks_a_case(emu, fault_runs, fault):
    """Each mistake, built into a copy of the statement, must put at least one case outside its bound (or its valid map)."""
    assert fault in vr.FAULTS
    _, good = vc.rows_of(7, 17, 23)
    _, bad = vc.rows_of(7, 17, 23, fault)                   # differs from `good` for roll_sign only
    broken = []
    for x, got in fault_runs["image"]:
        broken.append(_breaks(lambda: vc.check_values(got, vr.view_image(x, bad, fault), vc.image_bound(x, good), f"{fault}: image")))
    for flow, (got, valid) in fault_runs["flow"]:
        ref = vr.view_flow(flow, bad, vc.MIN_FORWARD, fault)
        broken.append(_breaks(lambda: vc.check_flow(got, valid, flow, good, f"{fault}: flow", ref=ref)))
    for faces, got in fault_runs["cube"]:
        broken.append(_breaks(lambda: vc.check_values(got, vr.cubemap_to_erp(faces, 32, 64, fault), vc.cube_bound(faces, 32, 64),
                                                      f"{fault}: cube")))
    broken.append(vr.cube_face(np.array(vc.TIES), fault).tolist() != vc.emu_faces(emu, vc.TIES).tolist())
    print(f"[viewport] seeded fault {fault}: breaks {sum(broken)} of {len(broken)} checks")
    assert any(broken), fault
    # and the unfaulted statement breaks none of them
    if fault == vr.FAULTS[0]:
        for x, got in fault_runs["image"]:
            vc.check_values(got, vr.view_image(x, good), vc.image_bound(x, good), "no fault: image")
        for flow, (got, valid) in fault_runs["flow"]:
            vc.check_flow(got, valid, flow, good, "no fault: flow")


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def _refusals(d):
    """Every refusal answers before a launch, so host pointers will do.  -1 = PF_ERR_BAD_ARG, -2 = PF_ERR_BAD_SHAPE."""
    F = ctypes.c_float
    buf = [ctypes.cast((ctypes.c_float * 4096)(), ctypes.c_void_p) for _ in range(3)]
    good = vr.table32(vr.cube_rows(4))

    def table(rows):
        return (F * rows.size)(*rows.reshape(-1).tolist())

    def image(t=good, V=6, B=1, C=1, H=8, W=16, form=0, i=buf[0], o=buf[1]):
        return d.pf_viewport_image(i, o, table(t) if t is not None else None, V, B, C, H, W, form, None)

    def flow(t=good, V=6, B=1, H=8, W=16, mf=0.1, i=buf[0], o=buf[1], v=buf[2]):
        return d.pf_viewport_flow(i, table(t) if t is not None else None, V, o, v, B, H, W, F(mf), None)

    def cube(B=1, C=1, s=4, H=8, W=16, i=buf[0], o=buf[1]):
        return d.pf_cubemap_to_erp(i, o, B, C, s, H, W, None)

    def changed(k, v, row=0):
        t = good.copy()
        t[row, k] = v
        return t

    for call in (image, flow):
        assert call(i=None) == -1 and call(o=None) == -1 and call(t=None) == -1            # null pointers
        assert call(o=buf[0]) == -1                                                        # in place
        assert call(V=0) == -2 and call(t=np.tile(good, (3, 1)), V=17) == -2               # V outside 1..16
        for f in (0.0, -1.0, np.inf, np.nan):
            assert call(t=changed(9, f)) == -1                                             # f <= 0 or not finite
        assert call(t=changed(0, np.nan, row=3)) == -1                                     # an R entry that is not finite
        assert call(t=changed(10, 0.0)) == -2 and call(t=changed(11, 2.5)) == -2           # sizes below 1 / no integer
        assert call(t=changed(10, 5.0, row=2)) == -2                                       # the views differ in size
        assert call(B=0) == -2 and call(H=0) == -2 and call(W=0) == -2
        assert call(B=10923) == -2 and call(B=65536, V=1) == -2                            # B * V above the grid limit
    assert image(C=0) == -2 and image(form=2) == -1
    assert flow(v=None) == -1 and flow(v=buf[1]) == -1
    for mf in (0.0, 1.0, -0.5, np.nan):
        assert flow(mf=mf) == -1
    assert cube(i=None) == -1 and cube(o=None) == -1 and cube(o=buf[0]) == -1
    assert cube(B=0) == -2 and cube(C=0) == -2 and cube(s=0) == -2 and cube(H=0) == -2 and cube(W=0) == -2 and cube(B=65536) == -2


def test_refusals_answer_without_a_gpu(emu):
    import __graft_entry__ as ge
    from prior_flow_amd import _lib
    _refusals(_lib.PfLib(ge.build_hip(), require_cuda=False)._dll)                # the built device library: nothing is launched
    _refusals(emu._dll)
    # through the emulation the accepted calls run: the same arguments without the fault
    t32 = vr.table32(vr.cube_rows(4))
    assert vc.run_image(emu, vc.make_image(1, 1, 8, 16, 1), t32).shape == (1, 6, 1, 4, 4)


def test_python_layer_refuses_cpu_tensors_and_bad_views():
    import torch

    from prior_flow_amd import projection as pj
    from prior_flow_amd._lib import PfError
    with pytest.raises(PfError):
        pj.ViewRenderer(1, 32, 64, pj.cube_faces(8), "cpu")
    with pytest.raises(PfError):
        pj.erp_to_cubemap(torch.zeros(1, 3, 32, 64), 8)
    with pytest.raises(PfError):
        pj.cubemap_to_erp(torch.zeros(1, 6, 3, 8, 8), 32, 64)
    for bad in (lambda: pj.Viewport(0, 0, 0, 180.0, 8, 8), lambda: pj.Viewport(0, 0, 0, 90.0, 0, 8), lambda: pj.View(np.eye(3), -1.0, 8, 8),
                lambda: pj.View(np.eye(2), 1.0, 8, 8)):
        with pytest.raises(PfError):
            bad()
