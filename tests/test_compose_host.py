"""Chained flows and point tracks without a GPU: the host emulation of pf_flow_compose / pf_track_points / pf_track_grid
(csrc/pf_elem.h, the code the device runs) against the float64 restatement of tests/compose_ref.py -- the constructed cases,
exact fields, seeded faults the check must catch, the refusals of the entry points and of the Python layer."""
import ctypes
import os

import numpy as np
import pytest
import torch

import compose_cases as cc
import compose_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_SO = os.path.join(ROOT, "tests", "emu", "libpf_emu.so")


@pytest.fixture(scope="module")
def emu():
    import emu_lib
    return emu_lib.load()


# ---- the constructed cases ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shape,wind", cc.DENSE)
def test_emulated_compose_matches_float64(emu, kind, shape, wind):
    figures = cc.check_dense_case(emu, kind, shape, wind)
    # the inputs exercise what they are meant to: the mask bit on 6..13 % of the pixels, the pole bit nowhere on `smooth` and on
    # 4..25 % of `seam` and `poles` (3.99 % on seam at 64x128)
    occl, pole = np.mean([f["occluded"] for f in figures]), np.mean([f["pole"] for f in figures])
    assert 0.06 <= occl <= 0.13, figures
    assert pole == 0.0 if kind == "smooth" else 0.035 <= pole <= 0.25, figures


@pytest.mark.parametrize("N", [1, 257])
@pytest.mark.parametrize("shape", cr.SHAPES[:2])
@pytest.mark.parametrize("kind", cr.KINDS)
def test_emulated_track_points_matches_float64(emu, kind, shape, N):
    figures = cc.check_sparse_case(emu, kind, shape, N)
    if N > 1:
        assert all(f["pole"] > 0 for f in figures) and any(f["occluded"] > 0 for f in figures)


def test_flow_stored_across_half_width(emu):
    """g's u around W/2, stored clipped: the taps are un-wrapped before they are blended."""
    for B, H, W in cr.SHAPES[:2]:
        f, g = cr.across_half_width(B, H, W)
        (out, st), = cc.run_dense(emu, [(f, None, g, None)])
        for b in range(B):
            ref = cr.reference_dense(f[b], g[b])
            cr.check(out[b], st[b], ref, None, f"across W/2 {H}x{W} image {b}")
            assert np.abs(np.abs(ref["gu"]) - W / 2).max() < 2.0            # every sample is a flow of about half a turn


def test_without_state_and_mask(emu):
    """NULL state_f reads as 0, NULL occ_g sets no mask bit, NULL state_out is not written."""
    B, H, W = 2, 17, 37
    f, g, _, _ = cr.inputs("poles", B, H, W, 1.5)
    (out, st), = cc.run_dense(emu, [(f, None, g, None)])
    for b in range(B):
        fig = cr.check(out[b], st[b], cr.reference_dense(f[b], g[b]), None, f"no state, image {b}")
        assert fig["occluded"] == 0.0 and fig["pole"] > 0
    ft, gt = torch.from_numpy(f), torch.from_numpy(g)
    o2 = torch.full_like(ft, float("nan"))
    emu.flow_compose([(ft, None, gt, None, o2, None)])
    assert np.array_equal(o2.numpy(), out)


def test_forms_agree_bitwise(emu):
    """In place (out = f, state_out = state_f) equals out of place; two jobs in one launch equal two launches."""
    for B, H, W in cr.SHAPES[:2]:
        f, g, state, occ = cr.inputs("seam", B, H, W, -3.0)
        f2, g2, state2, occ2 = cr.inputs("poles", B, H, W, 1.5)
        (o, s), = cc.run_dense(emu, [(f, state, g, occ)])
        (oi, si), = cc.run_dense(emu, [(f, state, g, occ)], in_place=True)
        assert np.array_equal(o.view(np.uint32), oi.view(np.uint32)) and np.array_equal(s, si)
        (p, t), = cc.run_dense(emu, [(f2, state2, g2, occ2)])
        both = cc.run_dense(emu, [(f, state, g, occ), (f2, state2, g2, occ2)])
        for got, want in zip(both, ((o, s), (p, t))):
            assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1], want[1])
        four = cc.run_dense(emu, [(f, state, g, occ), (f2, state2, g2, occ2), (f2, None, g, occ), (f, state2, g2, None)])
        assert np.array_equal(four[0][0].view(np.uint32), o.view(np.uint32)) and np.array_equal(four[1][1], t)


def test_tracker_on_the_grid_equals_dense_compose(emu):
    """pf_track_grid writes the pixel centres; one step of a PointTracker from there is the grid plus the dense compose of a zero
    flow, bit for bit, with the same state; at equal positions the two forms set the same bits whatever f is."""
    from prior_flow_amd.tracks import PointTracker, compose_flow
    for B, H, W in cr.SHAPES[:2]:
        _, g, _, occ = cr.inputs("seam", B, H, W, 0.0)
        gt, ot = torch.from_numpy(g), torch.from_numpy(occ)
        trk = PointTracker.grid(B, H, W, "cpu", lib=emu)
        grid = cc.grid_np(B, H, W)
        assert np.array_equal(trk.pos.numpy(), grid)
        pos, state = trk.push(gt, ot)
        flow, st = compose_flow(torch.zeros(B, 2, H, W), gt, occ_g=ot, lib=emu)
        want = grid + flow.numpy().reshape(B, 2, H * W).transpose(0, 2, 1)          # fp32: the same addition the tracker makes
        assert np.array_equal(pos.numpy().view(np.uint32), want.view(np.uint32))
        assert np.array_equal(state.numpy(), st.numpy().reshape(B, H * W))
        # a second step: the dense chain stores the displacement, the tracker the position, so the values differ by roundings
        #  -- but a tracker placed at the dense form's own p = (x, y) + f decides the same bits
        f, g2, _, occ2 = cr.inputs("poles", B, H, W, 1.5)
        p = grid + f.reshape(B, 2, H * W).transpose(0, 2, 1)
        t2 = PointTracker(torch.from_numpy(p), H, W, lib=emu)
        _, s2 = t2.push(torch.from_numpy(g2), torch.from_numpy(occ2))
        _, sd = compose_flow(torch.from_numpy(f), torch.from_numpy(g2), occ_g=torch.from_numpy(occ2), lib=emu)
        assert np.array_equal(s2.numpy(), sd.numpy().reshape(B, H * W))


# ---- exact fields ------------------------------------------------------------------------------------------------------------
def test_yaw_rotation_accumulates_with_its_winding(emu):
    """A constant non-integer u per step (a yaw rotation) over 8 steps: forward_u = sum c_t within the bound -- more than one turn
    of the panorama, so a chain that wrapped its u fails --, v = 0 and state 0 everywhere."""
    from prior_flow_amd.tracks import FlowChain
    B, H, W = 1, 24, 48
    steps = [7.3, 11.6, 9.25, 13.1, 12.7, 5.9, 10.45, 8.8]
    assert sum(steps) > 1.5 * W
    chain = FlowChain(B, H, W, "cpu", lib=emu)
    total = 0.0
    for c in steps:
        g = torch.zeros(B, 2, H, W)
        g[:, 0] = c
        chain.push(g)
        total += float(np.float32(c))
    assert chain.length == 8 and chain.backward is None
    u, v = chain.forward[0, 0].numpy().astype(np.float64), chain.forward[0, 1].numpy()
    # per step: the sample of a constant field (spread S = 0) and one addition of numbers below `total`
    tol = len(steps) * 4 * 2.0 ** -23 * (W + total + max(steps))
    print("yaw: worst error", np.abs(u - total).max(), "bound", tol)
    assert np.abs(u - total).max() <= tol
    assert not v.any() and not chain.state.numpy().any() and bool(chain.visible.all())


def test_affine_field_composes_to_its_closed_form(emu):
    """u = c + d y, v = a y + b composed with itself: away from the clamped rows the bilinear sample of an affine field is the
    field, so out_u = 2c + d (y + y'), out_v = v + a y' + b with y' = y + v."""
    B, H, W = 1, 24, 48
    a, b, c, d = 0.125, -1.5, 30.2, 0.75               # u up to 47: past the seam and past W/2
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    f = np.stack([c + d * y, a * y + b])[None].astype(np.float32)
    (out, st), = cc.run_dense(emu, [(f, None, f, None)])
    f64 = f[0].astype(np.float64)
    y1 = y + f64[1]
    inner = (y1 >= 0) & (y1 <= H - 1)
    want = np.stack([f64[0] + (np.float32(c) + np.float32(d) * y1), f64[1] + (np.float32(a) * y1 + np.float32(b))])
    ref = cr.reference_dense(f[0], f[0])
    err = np.abs(out[0] - want).max(0)
    print("affine: worst error / bound", (err[inner] / ref["tol"][inner]).max(), "rows", int(inner[:, 0].sum()))
    assert inner[:, 0].sum() >= H - 4 and (err[inner] <= ref["tol"][inner]).all()
    assert not st[0][inner].any()
    cr.check(out[0], st[0], ref, None, "affine")


# ---- the check catches what it must ------------------------------------------------------------------------------------------
def _half_mask_case():
    """Points exactly between an occluded and a free pixel: f_u = 0.5 on a zero g, the mask on every other column -> m = 0.5
    exactly (all of it exact in fp32)."""
    H, W = 8, 16
    f = np.zeros((2, H, W), np.float32)
    f[0] = 0.5
    occ = np.zeros((H, W), np.uint8)
    occ[:, ::2] = 1
    return f, np.zeros((2, H, W), np.float32), occ


@pytest.mark.parametrize("fault", cr.FAULTS)
def test_check_catches_seeded_fault(fault):
    """Each deviation from the statement, seeded into a copy of the restatement, fails `check` on at least one case (and the
    restatement itself passes every one of them)."""
    caught = 0
    cases = [(k, s, w) for k in cr.KINDS for s in cr.SHAPES[:2] for w in (0.0, 1.5)]
    for kind, (B, H, W), wind in cases:
        f, g, state, occ = cr.inputs(kind, B, H, W, wind)
        ref = cr.reference_dense(f[0], g[0], state[0], occ[0])
        cr.check(ref["out"].astype(np.float32), ref["state"], ref, state[0], "self")
        bad = cr.reference_dense(f[0], g[0], state[0], occ[0], fault=fault)
        try:
            cr.check(bad["out"].astype(np.float32), bad["state"], ref, state[0], f"{fault} {kind}")
        except AssertionError:
            caught += 1
    for B, H, W in cr.SHAPES[:2]:
        f, g = cr.across_half_width(B, H, W)
        ref = cr.reference_dense(f[0], g[0])
        cr.check(ref["out"].astype(np.float32), ref["state"], ref, None, "across self")
        bad = cr.reference_dense(f[0], g[0], fault=fault)
        try:
            cr.check(bad["out"].astype(np.float32), bad["state"], ref, None, f"{fault} across W/2")
        except AssertionError:
            caught += 1
    f, g, occ = _half_mask_case()
    ref = cr.reference_dense(f, g, None, occ)
    assert (ref["m"] == 0.5).all() and (ref["bits"] == cr.OCCLUDED).all()
    cr.check(ref["out"].astype(np.float32), ref["state"], ref, None, "half self", exact=True)
    bad = cr.reference_dense(f, g, None, occ, fault=fault)
    try:
        cr.check(bad["out"].astype(np.float32), bad["state"], ref, None, f"{fault} half", exact=True)
    except AssertionError:
        caught += 1
    assert caught >= 1, fault
    if fault == "gt":
        assert caught == 1          # only the case that sits exactly at 0.5 tells > from >=


def test_half_mask_is_occluded(emu):
    """m = 0.5 exactly counts as occluded (>=), on the emulation of the device code."""
    f, g, occ = _half_mask_case()
    (out, st), = cc.run_dense(emu, [(f[None], None, g[None], occ[None])])
    cr.check(out[0], st[0], cr.reference_dense(f, g, None, occ), None, "half", exact=True)
    assert (st == cr.OCCLUDED).all()


def test_non_finite_values_are_flagged_and_add_nothing(emu):
    B, H, W = 1, 17, 37
    f, g, state, occ = cr.inputs("smooth", B, H, W, 0.0)
    f, g = f.copy(), g.copy()
    f[0, 0, 3, 4] = np.nan
    f[0, 1, 5, 6] = np.inf
    g[0, 0, 10, 20] = np.nan
    g[0, 1, 12, 8] = -np.inf
    (out, st), = cc.run_dense(emu, [(f, state, g, occ)])
    ref = cr.reference_dense(f[0], g[0], state[0], occ[0])
    fig = cr.check(out[0], st[0], ref, state[0], "non-finite")
    assert ref["bad"].sum() >= 4 and (st[0][ref["bad"]] & cr.NONFINITE).all() and fig["wrong_decided"] == 0
    assert not (st[0][~ref["bad"]] & cr.NONFINITE & ~state[0][~ref["bad"]]).any()
    pos = np.array([[[np.nan, 3.0], [5.0, np.inf], [10.2, 20.4]]], np.float32)
    p, s = cc.run_points(emu, pos, np.zeros((1, 3), np.uint8), g, None)
    assert np.isnan(p[0, 0, 0]) and p[0, 0, 1] == 3.0 and p[0, 1, 0] == 5.0 and np.isinf(p[0, 1, 1])
    assert s[0, 0] & cr.NONFINITE and s[0, 1] & cr.NONFINITE and not s[0, 2] & cr.NONFINITE


# ---- FlowChain and PointTracker on the emulation -------------------------------------------------------------------------------
def test_flow_chain_is_compose_step_by_step(emu):
    from prior_flow_amd.tracks import FlowChain, compose_flow
    from prior_flow_amd.video import BidirectionalFlow
    B, H, W = 2, 24, 48
    chain = FlowChain(B, H, W, "cpu", lib=emu)
    fw = st = bw = bst = None
    for t, kind in enumerate(cr.KINDS):
        f, g, _, occ = cr.inputs(kind, B, H, W, 0.0)
        r = BidirectionalFlow(torch.from_numpy(f), torch.from_numpy(g), torch.from_numpy(occ), torch.from_numpy(np.roll(occ, 5, 2).copy()),
                              None, None)
        chain.push(r)
        if t == 0:
            z = torch.zeros(B, 2, H, W)
            fw, st = compose_flow(z, r.forward, occ_g=r.occ_forward, lib=emu)
            bw, bst = compose_flow(r.backward, z, state_f=r.occ_backward, lib=emu)
            assert torch.equal(fw, r.forward) and torch.equal(bw, r.backward)       # the first pair is the pair itself
        else:
            fw, st = compose_flow(fw, r.forward, state_f=st, occ_g=r.occ_forward, lib=emu)
            bw, bst = compose_flow(r.backward, bw, state_f=r.occ_backward, occ_g=bst, lib=emu)
        assert chain.length == t + 1
        assert torch.equal(chain.forward, fw) and torch.equal(chain.state, st)
        assert torch.equal(chain.backward, bw) and torch.equal(chain.backward_state, bst)
    assert 0.0 < float(chain.visible.float().mean()) < 1.0
    for t in [chain._fw] + chain._bw:
        t.fill_(float("nan"))
    for t in [chain._fw_state] + chain._bw_state:
        t.fill_(255)
    chain.reset()
    assert chain.length == 0
    f, g, _, occ = cr.inputs("smooth", B, H, W, 0.0)
    chain.push(BidirectionalFlow(torch.from_numpy(f), torch.from_numpy(g), None, None, None, None))
    assert torch.equal(chain.forward, torch.from_numpy(f)) and torch.equal(chain.backward, torch.from_numpy(g))
    # nothing of the poisoned chain is left: the forward state is clean, the backward state is that of the pair alone
    assert not chain.state.any()
    assert torch.equal(chain.backward_state, compose_flow(torch.from_numpy(g), torch.zeros(B, 2, H, W), lib=emu)[1])


def test_point_tracker_history_and_wrapping(emu):
    from prior_flow_amd.tracks import PointTracker
    B, H, W, N = 1, 24, 48, 5
    g = torch.zeros(B, 2, H, W)
    g[:, 0] = 20.5
    pts = torch.tensor([[[1.0, 2.0], [47.5, 3.0], [10.25, 23.0], [0.0, 0.0], [30.0, 11.5]]])
    trk = PointTracker(pts, H, W, history=3, lib=emu)
    seen = []
    for _ in range(5):
        pos, state = trk.push(g)
        seen.append(pos.clone())
    assert torch.equal(pos[..., 0], pts[..., 0] + 5 * 20.5) and torch.equal(pos[..., 1], pts[..., 1]) and not state.any()
    assert torch.equal(trk.pos_wrapped[..., 0], torch.remainder(pos[..., 0], 48.0)) and float(trk.pos_wrapped[..., 0].max()) < W
    assert tuple(trk.history.shape) == (3, B, N, 2) and torch.equal(trk.trajectory(), torch.stack(seen[-3:]))
    assert torch.equal(pts, torch.tensor([[[1.0, 2.0], [47.5, 3.0], [10.25, 23.0], [0.0, 0.0], [30.0, 11.5]]]))     # the caller's points stay


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments(emu):
    """PF_ERR_* before any launch, in the emulation build and in the device build when it has been built (no GPU needed)."""
    from prior_flow_amd import _lib
    libs = [ctypes.CDLL(EMU_SO)]
    if os.path.exists(_lib.LIB_PATH):
        libs.append(ctypes.CDLL(_lib.LIB_PATH))
    H, W = 4, 8
    bufs = [(ctypes.c_float * (2 * H * W))() for _ in range(8)]
    f, g, out, sf, occ, so, f2, o2 = [ctypes.cast(b, ctypes.c_void_p).value for b in bufs]
    vp, ci = ctypes.c_void_p, ctypes.c_int

    def jobs(*rows):
        arr = (_lib.ComposeJob * max(len(rows), 1))()
        for q, row in zip(arr, rows):
            q.f, q.state_f, q.g, q.occ_g, q.out, q.state_out = row
        return arr

    good = (f, sf, g, occ, out, so)
    for dll in libs:
        fc = dll.pf_flow_compose
        fc.argtypes, fc.restype = [ctypes.POINTER(_lib.ComposeJob), ci, ci, ci, ci, vp], ci
        assert fc(None, 1, 1, H, W, None) == -1
        assert fc(jobs(good), 0, 1, H, W, None) == -1 and fc(jobs(good), 5, 1, H, W, None) == -1      # njobs outside 1..4
        for i in (0, 2, 4):                                                                     # NULL f, g, out
            assert fc(jobs(good[:i] + (None,) + good[i + 1:]), 1, 1, H, W, None) == -1, i
        assert fc(jobs((f, sf, g, occ, g, so)), 1, 1, H, W, None) == -1                         # out == g
        assert fc(jobs((f, sf, g, occ, out, occ)), 1, 1, H, W, None) == -1                      # state_out == occ_g
        assert fc(jobs(good, (f2, None, g, None, out, None)), 2, 1, H, W, None) == -1           # two jobs, one output
        assert fc(jobs(good, (f2, None, out, None, o2, None)), 2, 1, H, W, None) == -1          # a job reads another's output
        for B_, H_, W_ in ((0, H, W), (1, 0, W), (1, H, 0), (-1, H, W), (1, 1 << 15, 1 << 15)):
            assert fc(jobs(good), 1, B_, H_, W_, None) == -2, (B_, H_, W_)
        tp = dll.pf_track_points
        tp.argtypes, tp.restype = [vp] * 4 + [ci] * 4 + [vp], ci
        for i in (0, 1, 2):                                                                     # NULL pos, state, flow
            a = [f, sf, g, occ]
            a[i] = None
            assert tp(*a, 1, 2, H, W, None) == -1, i
        for B_, N_, H_, W_ in ((0, 2, H, W), (1, 0, H, W), (1, 2, 0, W), (1, 2, H, 0), (1, 2, 1 << 15, 1 << 15)):
            assert tp(f, sf, g, occ, B_, N_, H_, W_, None) == -2
        tg = dll.pf_track_grid
        tg.argtypes, tg.restype = [vp, ci, ci, ci, vp], ci
        assert tg(None, 1, H, W, None) == -1
        for B_, H_, W_ in ((0, H, W), (1, 0, W), (1, H, 0), (1, 1 << 15, 1 << 15)):
            assert tg(f, B_, H_, W_, None) == -2
        # the same calls without the fault run (host build only: the device build would launch)
    d = libs[0]
    assert d.pf_flow_compose(jobs(good), 1, 1, H, W, None) == 0
    assert d.pf_flow_compose(jobs((f, sf, g, occ, f, sf)), 1, 1, H, W, None) == 0               # in place is allowed
    assert d.pf_track_grid(f, 1, H, W // 2, None) == 0


def test_python_layer_refuses_cpu_tensors_and_bad_shapes(emu):
    from prior_flow_amd.tracks import FlowChain, PointTracker, compose_flow
    from prior_flow_amd._lib import PfError
    z = torch.zeros(1, 2, 8, 16)
    with pytest.raises(PfError):
        compose_flow(z, z.clone())                              # no CPU path
    with pytest.raises(PfError):
        FlowChain(1, 8, 16, "cpu")
    with pytest.raises(PfError):
        PointTracker(torch.zeros(1, 3, 2), 8, 16)
    with pytest.raises(PfError):
        compose_flow(z, torch.zeros(1, 2, 8, 17), lib=emu)
    with pytest.raises(PfError):
        compose_flow(torch.zeros(1, 3, 8, 16), z, lib=emu)
    with pytest.raises(PfError):
        compose_flow(z, z.clone(), occ_g=torch.zeros(1, 8, 16), lib=emu)            # a float mask
    with pytest.raises(PfError):
        compose_flow(z, z.clone(), state_f=torch.zeros(1, 8, 15, dtype=torch.uint8), lib=emu)
    with pytest.raises(PfError):
        compose_flow(z, z, out=(z, torch.zeros(1, 8, 16, dtype=torch.uint8)), lib=emu)       # out over g
    with pytest.raises(PfError):
        emu.flow_compose([])
    with pytest.raises(PfError):
        emu.flow_compose([(z, None, z.clone(), None, z.clone(), None)] * 5)
    chain = FlowChain(1, 8, 16, "cpu", lib=emu)
    with pytest.raises(PfError):
        chain.push(torch.zeros(1, 2, 8, 17))
    with pytest.raises(PfError):
        chain.push(torch.zeros(2, 8, 16))
    with pytest.raises(PfError):
        PointTracker(torch.zeros(3, 2), 8, 16, lib=emu)
    trk = PointTracker(torch.zeros(1, 3, 2), 8, 16, lib=emu)
    with pytest.raises(PfError):
        trk.push(torch.zeros(1, 2, 8, 17))
    with pytest.raises(PfError):
        trk.push(z, occ=torch.zeros(1, 8, 16))
    with pytest.raises(PfError):
        trk.trajectory()
