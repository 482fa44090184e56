"""Perspective viewports and cube maps on an MI355X: pf_viewport_image, pf_viewport_flow and
pf_cubemap_to_erp against the float64 statement (tests/viewport_ref.py) under the derived per-pixel bounds of
tests/viewport_cases.py, against the host emulation, twice and batched for equal bytes, between guard rows (every runner of
viewport_cases checks them), ViewRenderer inside a captured graph, and behind a FlowStream step.  Run with ``-m gpu``.

The figures measured on the device are in DESIGN.md section 15.
"""
import argparse

import numpy as np
import pytest
import torch

import golden_cases as gc
import viewport_cases as vc
import viewport_ref as vr

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def lib():
    from prior_flow_amd._lib import load
    return load()


@pytest.fixture(scope="module")
def emu():
    import __graft_entry__ as ge
    from prior_flow_amd import _lib
    so = ge.build_emu_viewport()
    keep = ("pf_viewport_image", "pf_viewport_flow", "pf_cubemap_to_erp")
    return _lib.PfLib(so, require_cuda=False, optional=tuple(n for n in _lib.EXPORTS if n not in keep))


# ---- values ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", vc.VIEW_SIZES)
@pytest.mark.parametrize("H,W", vc.PANORAMAS)
def test_images_hold_the_bounds(lib, emu, H, W, h, w):
    worst, apart, bytes_apart = 0.0, 0.0, 0
    for V in vc.VIEW_SETS:
        for B, C, form in vc.IMAGE_FORMS:
            got, r = vc.image_case(lib, H, W, h, w, V, B, C, form, DEV)
            twin, _ = vc.image_case(emu, H, W, h, w, V, B, C, form)
            if form == "f32":
                worst, apart = max(worst, r), max(apart, float(np.abs(got - twin).max()))
            else:
                assert np.abs(got.astype(int) - twin.astype(int)).max() <= 1
                bytes_apart += int((got != twin).sum())
    print(f"[viewport] device images {H}x{W} -> {h}x{w}: worst ratio {worst:.3f}; from the emulation at most {apart:.3e} (values 0..255), "
          f"{bytes_apart} bytes")


@pytest.mark.parametrize("h,w", vc.VIEW_SIZES)
@pytest.mark.parametrize("H,W", vc.PANORAMAS)
def test_flows_hold_the_bounds(lib, emu, H, W, h, w):
    worst, apart = 0.0, 0.0
    for V in vc.VIEW_SETS:
        for kind in vc.FLOW_KINDS:
            got, valid, r = vc.flow_case(lib, H, W, h, w, V, kind, DEV)
            twin, tvalid, _ = vc.flow_case(emu, H, W, h, w, V, kind)
            both = (valid == 1) & (tvalid == 1)
            worst = max(worst, r)
            apart = max(apart, float(np.abs(got - twin)[np.broadcast_to(both[:, :, None], got.shape)].max(initial=0.0)))
            if kind == "zero":
                assert not got.any() and (valid == 1).all()                      # exactly zero, every valid bit
    print(f"[viewport] device flows {H}x{W} -> {h}x{w}: worst ratio {worst:.3f}; from the emulation at most {apart:.3e} px")


@pytest.mark.parametrize("s", vc.CUBE_SIZES)
def test_cube_maps_hold_the_bounds(lib, emu, s):
    worst, apart = 0.0, 0.0
    for B, C in ((1, 1), (2, 3)):
        got, r = vc.cube_case(lib, s, 32, 64, B, C, DEV)
        twin, _ = vc.cube_case(emu, s, 32, 64, B, C)
        worst, apart = max(worst, r), max(apart, float(np.abs(got - twin).max()))
    x = vc.make_image(2, 3, 32, 64, seed=s)
    t32 = vr.table32(vr.cube_rows(s))
    got = vc.run_image(lib, x, t32, DEV)
    worst = max(worst, vc.check_values(got, vr.view_image(x, t32), vc.image_bound(x, t32), f"ERP 32x64 -> cube {s} on {DEV}"))
    print(f"[viewport] device cube {s}: worst ratio {worst:.3f}; from the emulation at most {apart:.3e}")


# ---- determinism -------------------------------------------------------------------------------------------------------------
def test_two_launches_and_the_batch_give_equal_bytes(lib):
    H, W, h, w, V = 40, 72, 17, 23, 7
    _, t32 = vc.rows_of(V, h, w)
    x, u8 = vc.make_image(2, 3, H, W, seed=9), vc.make_u8(2, 3, H, W, seed=9)
    flow = vc.make_flow("smooth_nan", 2, H, W, seed=2)
    faces = vc.make_faces(2, 3, 12, seed=4)
    for run, data in ((lambda a: [vc.run_image(lib, a, t32, DEV)], x), (lambda a: [vc.run_image(lib, a, t32, DEV)], u8),
                      (lambda a: list(vc.run_flow(lib, a, t32, device=DEV)), flow), (lambda a: [vc.run_cube(lib, a, 32, 64, DEV)], faces)):
        first, second = run(data), run(data)
        for p, q in zip(first, second):
            assert np.array_equal(p.view(np.uint8), q.view(np.uint8))
        for b in range(2):
            for p, q in zip(first, run(data[b:b + 1])):
                assert np.array_equal(p[b:b + 1].view(np.uint8), q.view(np.uint8)), b


# ---- ViewRenderer --------------------------------------------------------------------------------------------------------------
def _views(h, w, V=4):
    from prior_flow_amd.projection import Viewport
    return [Viewport(y, p, r, fov, h, w) for y, p, r, fov in vc.VIEW_SETS[V]]


def test_python_interface(lib):
    from prior_flow_amd import projection as pj
    from prior_flow_amd._lib import PfError
    B, H, W, h, w = 2, 32, 64, 17, 23
    _, t32 = vc.rows_of(4, h, w)
    r = pj.ViewRenderer(B, H, W, _views(h, w), DEV)
    x, u8, flow = vc.make_image(B, 3, H, W, 1), vc.make_u8(B, 3, H, W, 1), vc.make_flow("smooth", B, H, W, 1)
    got = r.image(torch.from_numpy(x).cuda())
    assert tuple(got.shape) == (B, 4, 3, h, w) and np.array_equal(got.cpu().numpy(), vc.run_image(lib, x, t32, DEV))
    got8 = r.image(torch.from_numpy(u8).cuda())
    assert tuple(got8.shape) == (B, 4, h, w, 3) and got8.dtype == torch.uint8
    assert np.array_equal(got8.cpu().numpy(), vc.run_image(lib, u8, t32, DEV))
    fv, valid = r.flow(torch.from_numpy(flow).cuda())
    want = vc.run_flow(lib, flow, t32, device=DEV)
    assert np.array_equal(fv.cpu().numpy(), want[0]) and np.array_equal(valid.cpu().numpy(), want[1])
    own = torch.zeros_like(fv)
    assert r.flow(torch.from_numpy(flow).cuda(), out=own)[0] is own and torch.equal(own, fv)
    for bad in (lambda: r.image(torch.from_numpy(x)), lambda: r.flow(torch.from_numpy(flow)), lambda: r.image(torch.zeros(B, 3, H, W + 1).cuda()),
                lambda: r.flow(torch.zeros(B, 2, H, W, dtype=torch.float64).cuda()), lambda: r.image(torch.zeros(B, 3, H, W).cuda().half()),
                lambda: r.flow(torch.zeros(B, 2, H, W).cuda(), out=torch.zeros(B, 4, 2, h, w + 1).cuda()),
                lambda: pj.ViewRenderer(B, H, W, _views(h, w) + _views(16, 16), DEV), lambda: pj.ViewRenderer(B, H, W, [], DEV),
                lambda: pj.ViewRenderer(B, H, W, _views(h, w), DEV, min_forward=0.0)):
        with pytest.raises(PfError):
            bad()


@pytest.mark.parametrize("s", vc.CUBE_SIZES)
def test_cube_round_trip_is_the_statements(lib, s):
    """erp_to_cubemap then cubemap_to_erp on a smooth frame against the statement's round trip (not against the frame: the round
    trip is a resampling)."""
    from prior_flow_amd import projection as pj
    x = vc.make_image(2, 3, 32, 64, seed=30 + s)
    t32 = vr.table32(vr.cube_rows(s))
    faces = pj.erp_to_cubemap(torch.from_numpy(x).cuda(), s)
    assert tuple(faces.shape) == (2, 6, 3, s, s)
    back = pj.cubemap_to_erp(faces, 32, 64)
    f_np = faces.cpu().numpy()
    vc.check_values(f_np, vr.view_image(x, t32), vc.image_bound(x, t32), f"erp_to_cubemap {s}")
    # the second step is held to its bound on the device's own faces; the whole round trip to both budgets
    vc.check_values(back.cpu().numpy(), vr.cubemap_to_erp(f_np, 32, 64), vc.cube_bound(f_np, 32, 64), f"cubemap_to_erp {s}")
    trip = vr.cubemap_to_erp(vr.view_image(x, t32), 32, 64)
    carried = vr.cubemap_to_erp(np.abs(vc.image_bound(x, t32)), 32, 64)          # the first step's bound through the (convex) second
    vc.check_values(back.cpu().numpy(), trip, vc.cube_bound(vr.view_image(x, t32), 32, 64) + carried, f"round trip through cube {s}")


def test_renderer_captured_equals_eager_and_allocates_nothing(lib):
    from prior_flow_amd.projection import ViewRenderer
    B, H, W, h, w = 2, 40, 72, 17, 23
    xs = [torch.from_numpy(vc.make_image(B, 3, H, W, seed=s)).cuda() for s in (41, 42, 43)]
    us = [torch.from_numpy(vc.make_u8(B, 3, H, W, seed=s)).cuda() for s in (41, 42, 43)]
    fs = [torch.from_numpy(vc.make_flow(k, B, H, W, seed=5)).cuda() for k in ("smooth", "smooth_nan", "u_half")]
    eager = ViewRenderer(B, H, W, _views(h, w), DEV)
    want = []
    for x, u, f in zip(xs, us, fs):
        fv, valid = eager.flow(f)
        want.append((eager.image(x).clone(), eager.image(u).clone(), fv.clone(), valid.clone()))
    r = ViewRenderer(B, H, W, _views(h, w), DEV)
    r.prepare(3)
    r.prepare(3, torch.uint8)
    x_in, u_in, f_in = torch.zeros_like(xs[0]), torch.zeros_like(us[0]), torch.zeros_like(fs[0])
    r.image(x_in); r.image(u_in); r.flow(f_in)           # warm-up outside the capture
    torch.cuda.synchronize()
    events = lambda: torch.cuda.memory_stats()["allocation.all.allocated"]      # noqa: E731
    before, n_before = torch.cuda.memory_allocated(), events()
    for _ in range(3):
        r.image(x_in); r.image(u_in); r.flow(f_in)
    assert torch.cuda.memory_allocated() == before and events() == n_before      # construction and prepare, then no allocation
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        n0 = events()
        img, img8 = r.image(x_in), r.image(u_in)
        fv, valid = r.flow(f_in)
        n1 = events()
    assert n1 == n0, (n0, n1)
    for i in (1, 2, 0):                                  # new inputs in the same buffers
        x_in.copy_(xs[i]); u_in.copy_(us[i]); f_in.copy_(fs[i])
        g.replay()
        torch.cuda.synchronize()
        for got, w_ in zip((img, img8, fv, valid), want[i]):
            assert torch.equal(got, w_)


# ---- composition with the stream ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    from prior_flow_amd.modules import state_dict_shapes
    from prior_flow_amd.prior_raft import PriOr_RAFT
    m = PriOr_RAFT(argparse.Namespace(mixed_precision=False, dropout=0.0, alternate_corr=False))
    m.load_state_dict(gc.det_state_dict(state_dict_shapes()), strict=True)
    return m.cuda().eval()


def test_stream_then_views(model):
    """A cold FlowStream step at 128x256 feeds ViewRenderer.flow; the views agree with the statement on the stream's own flow."""
    from prior_flow_amd.projection import ViewRenderer
    from prior_flow_amd.video import FlowStream
    B, H, W, h, w = 1, 128, 256, 17, 23
    f0, _ = gc.synthetic_pair(B, H, W, seed=5)
    frames = [torch.roll(f0, shifts=(t, 3 * t), dims=(2, 3)).cuda() for t in range(2)]
    r = ViewRenderer(B, H, W, _views(h, w), DEV)
    _, t32 = vc.rows_of(4, h, w)
    with torch.no_grad():
        s = FlowStream(model, iters=4, warm_start=False)
        assert s(frames[0]) is None
        flow = s(frames[1]).contiguous()
        fv, valid = r.flow(flow)
        img = r.image(frames[1])
    torch.cuda.synchronize()
    flow_np = flow.cpu().numpy()
    assert np.isfinite(flow_np).all()
    vc.check_flow(fv.cpu().numpy(), valid.cpu().numpy(), flow_np, t32, "FlowStream step 128x256 -> 4 x 17x23")
    x = frames[1].cpu().numpy()
    vc.check_values(img.cpu().numpy(), vr.view_image(x, t32), vc.image_bound(x, t32), "the step's frame 128x256 -> 4 x 17x23")
