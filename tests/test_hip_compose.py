"""Chained flows and point tracks on an MI355X: pf_flow_compose (both launch forms), pf_track_points and pf_track_grid on the
device against the float64 restatement (tests/compose_ref.py) and, bit for bit, against the host emulation of the same
functions; FlowChain behind a bidirectional FlowStream, eager and captured.  Run with ``-m gpu``."""
import argparse

import numpy as np
import pytest
import torch

import compose_cases as cc
import compose_ref as cr
import golden_cases as gc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def emu():
    import emu_lib
    return emu_lib.load()


@pytest.fixture(scope="module")
def lib():
    from prior_flow_amd._lib import load
    return load()


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.mark.parametrize("kind,shape,wind", cc.DENSE)
def test_compose_matches_float64_and_the_emulation(lib, emu, kind, shape, wind):
    """17x37 takes the element form, 24x48 and 64x128 four pixels per thread; every case holds the bounds and carries the
    emulation's bits (the same function, no contraction on either side)."""
    cc.check_dense_case(lib, kind, shape, wind, device="cuda")
    B, H, W = shape
    f, g, state, occ = cr.inputs(kind, B, H, W, wind)
    for in_place in (False, True):
        (d_out, d_st), = cc.run_dense(lib, [(f, state, g, occ)], device="cuda", in_place=in_place)
        (h_out, h_st), = cc.run_dense(emu, [(f, state, g, occ)])
        assert np.array_equal(bits(d_out), bits(h_out)) and np.array_equal(d_st, h_st), in_place


def test_compose_jobs_of_one_launch(lib, emu):
    """Four jobs in one launch (with and without state and mask) equal the emulation's; so does a launch whose maps are not
    16-byte aligned at a width that is a multiple of 4 (element form), and the flow stored across W/2."""
    for B, H, W in cr.SHAPES[:2]:
        f, g, state, occ = cr.inputs("seam", B, H, W, -3.0)
        f2, g2, state2, occ2 = cr.inputs("poles", B, H, W, 1.5)
        jobs = [(f, state, g, occ), (f2, state2, g2, occ2), (f2, None, g, occ), (f, state2, g2, None)]
        for dev, host in zip(cc.run_dense(lib, jobs, device="cuda"), cc.run_dense(emu, jobs)):
            assert np.array_equal(bits(dev[0]), bits(host[0])) and np.array_equal(dev[1], host[1])
        fa, ga = cr.across_half_width(B, H, W)
        (out, st), = cc.run_dense(lib, [(fa, None, ga, None)], device="cuda")
        (h_out, h_st), = cc.run_dense(emu, [(fa, None, ga, None)])
        for b in range(B):
            cr.check(out[b], st[b], cr.reference_dense(fa[b], ga[b]), None, f"across W/2 {H}x{W} image {b}")
        assert np.array_equal(bits(out), bits(h_out)) and np.array_equal(st, h_st)
    B, H, W = 2, 24, 48
    f, g, state, occ = cr.inputs("seam", B, H, W, 1.5)
    n = f.size
    buf = torch.zeros(n + 1, device="cuda")
    ft = buf[1:].view(B, 2, H, W)                       # 4 bytes past a 16-byte boundary
    ft.copy_(torch.from_numpy(f))
    out, st = torch.empty_like(ft), torch.empty(B, H, W, dtype=torch.uint8, device="cuda")
    lib.flow_compose([(ft, torch.from_numpy(state).cuda(), torch.from_numpy(g).cuda(), torch.from_numpy(occ).cuda(), out, st)])
    (h_out, h_st), = cc.run_dense(emu, [(f, state, g, occ)])
    assert np.array_equal(bits(out.cpu().numpy()), bits(h_out)) and np.array_equal(st.cpu().numpy(), h_st)


@pytest.mark.parametrize("N", [1, 257])
@pytest.mark.parametrize("shape", cr.SHAPES[:2])
@pytest.mark.parametrize("kind", cr.KINDS)
def test_track_points_matches_float64_and_the_emulation(lib, emu, kind, shape, N):
    cc.check_sparse_case(lib, kind, shape, N, device="cuda")
    B, H, W = shape
    _, g, _, occ = cr.inputs(kind, B, H, W, 0.0)
    pos, state = cc.sparse_points(B, H, W, N)
    d, h = cc.run_points(lib, pos, state, g, occ, device="cuda"), cc.run_points(emu, pos, state, g, occ)
    assert np.array_equal(bits(d[0]), bits(h[0])) and np.array_equal(d[1], h[1])


def test_tracker_on_the_grid_equals_dense_compose(lib):
    from prior_flow_amd.tracks import PointTracker, compose_flow
    for B, H, W in cr.SHAPES[:2]:
        _, g, _, occ = cr.inputs("seam", B, H, W, 0.0)
        gt, ot = torch.from_numpy(g).cuda(), torch.from_numpy(occ).cuda()
        trk = PointTracker.grid(B, H, W, "cuda", history=2)
        grid = cc.grid_np(B, H, W)
        assert np.array_equal(trk.pos.cpu().numpy(), grid)
        pos, state = trk.push(gt, ot)
        flow, st = compose_flow(torch.zeros(B, 2, H, W, device="cuda"), gt, occ_g=ot)
        want = grid + flow.cpu().numpy().reshape(B, 2, H * W).transpose(0, 2, 1)
        assert np.array_equal(bits(pos.cpu().numpy()), bits(want))
        assert np.array_equal(state.cpu().numpy(), st.cpu().numpy().reshape(B, H * W))
        assert torch.equal(trk.trajectory()[0], pos) and float(trk.pos_wrapped[..., 0].max()) < W


def test_python_layer_on_the_device():
    from prior_flow_amd._lib import PfError
    from prior_flow_amd.tracks import FlowChain, compose_flow
    z = torch.zeros(1, 2, 8, 16, device="cuda")
    with pytest.raises(PfError):
        compose_flow(z.cpu(), z.cpu())
    with pytest.raises(PfError):
        compose_flow(z, z.cpu())
    with pytest.raises(PfError):
        compose_flow(z, z, out=(z, torch.zeros(1, 8, 16, dtype=torch.uint8, device="cuda")))
    with pytest.raises(PfError):
        FlowChain(1, 8, 16, "cuda").push(z[:, :, :, ::2])            # not contiguous: push copies nothing


# ---- FlowChain behind the bidirectional stream ---------------------------------------------------------------------------------
def test_flow_chain_behind_the_stream_eager_captured_and_reset():
    """A four-frame 128x256 sequence, iters = 2, occlusion "plane": the chain equals compose_flow applied to the returned flows
    step by step; a captured push replayed twice gives the same bits; after reset() nothing of the first chain is left."""
    from prior_flow_amd.modules import state_dict_shapes
    from prior_flow_amd.prior_raft import PriOr_RAFT
    from prior_flow_amd.tracks import FlowChain, compose_flow
    from prior_flow_amd.video import BidirectionalFlow, FlowStream
    B, H, W = 1, 128, 256
    m = PriOr_RAFT(argparse.Namespace(mixed_precision=False, dropout=0.0, alternate_corr=False))
    m.load_state_dict(gc.det_state_dict(state_dict_shapes()), strict=True)
    m = m.cuda().eval()
    f0, _ = gc.synthetic_pair(B, H, W, seed=5)
    frames = [torch.roll(f0, shifts=(t, 3 * t), dims=(2, 3)).cuda() for t in range(4)]
    stream = FlowStream(m, iters=2, bidirectional=True, occlusion="plane")
    chain = FlowChain(B, H, W, "cuda")
    results, want = [], []
    fw = st = bw = bst = None
    with torch.no_grad():
        for frame in frames:
            r = stream(frame)
            if r is None:
                continue
            chain.push(r)
            results.append(BidirectionalFlow(*[t.clone() for t in r]))
            if fw is None:
                z = torch.zeros_like(r.forward)
                fw, st = compose_flow(z, r.forward, occ_g=r.occ_forward)
                bw, bst = compose_flow(r.backward, z, state_f=r.occ_backward)
            else:
                fw, st = compose_flow(fw, r.forward, state_f=st, occ_g=r.occ_forward)
                bw, bst = compose_flow(r.backward, bw, state_f=r.occ_backward, occ_g=bst)
            want.append((fw, st, bw, bst))
            assert torch.equal(chain.forward, fw) and torch.equal(chain.state, st)
            assert torch.equal(chain.backward, bw) and torch.equal(chain.backward_state, bst)
    assert chain.length == 3 and bool(torch.isfinite(chain.forward).all())
    assert chain.visible.dtype == torch.bool and torch.equal(chain.visible, chain.state == 0)
    # the third push again, captured: the chain is put back to its state after two pushes, the graph replayed -- twice
    cap = FlowChain(B, H, W, "cuda")
    cap.push(results[0]).push(results[1])
    saved = [t.clone() for t in [cap._fw, cap._fw_state] + cap._bw + cap._bw_state]
    cur = cap._cur
    src = BidirectionalFlow(*[torch.zeros_like(t) for t in results[2]])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        cap.push(src)                                   # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(side)
    cap._cur = cur
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap.push(src)
    for s, t in zip(src, results[2]):
        s.copy_(t)
    for _ in range(2):
        for t, s in zip([cap._fw, cap._fw_state] + cap._bw + cap._bw_state, saved):
            t.copy_(s)
        graph.replay()
        torch.cuda.synchronize()
        got = (cap.forward, cap.state, cap.backward, cap.backward_state)
        assert all(torch.equal(a, b) for a, b in zip(got, want[2]))
    # reset: poisoned buffers, then a fresh chain's first push
    for t in [chain._fw] + chain._bw:
        t.fill_(float("nan"))
    for t in [chain._fw_state] + chain._bw_state:
        t.fill_(255)
    chain.reset()
    chain.push(results[0])
    assert chain.length == 1
    assert all(torch.equal(a, b) for a, b in zip((chain.forward, chain.state, chain.backward, chain.backward_state), want[0]))
