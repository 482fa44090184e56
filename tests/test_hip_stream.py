"""Panoramic video inference on an MI355X: pf_forward_interpolate against the float64 brute force (tests/fwd_interp_ref.py), and
FlowStream (prior-flow_amd/video.py) against per-pair model(...) calls -- cold, warm-started, graph against eager, the frame
cache's reuse, isolation from plain calls, restarts, weight edits and every inference mode.  Run with ``-m gpu``."""
import argparse

import numpy as np
import pytest
import torch

import fwd_interp_ref as fref
import golden_cases as gc
import priorflow_oracle as po

pytestmark = pytest.mark.gpu

# cold stream against per-pair calls: fnet sees 2B images per launch in the stream, 4B in a pair (the bar of
# test_forward_batch2_matches_reference_and_is_batch_independent when the arithmetic of one image depends on the batch)
EPE_BATCH = 1e-5


@pytest.fixture(scope="module")
def params():
    from prior_flow_amd.modules import state_dict_shapes
    return gc.det_state_dict(state_dict_shapes())


def build(params, **kw):
    from prior_flow_amd.prior_raft import PriOr_RAFT
    m = PriOr_RAFT(argparse.Namespace(mixed_precision=kw.pop("mixed_precision", False), dropout=0.0,
                                      alternate_corr=kw.pop("alternate_corr", False)))
    m.load_state_dict(params, strict=True)
    return m.cuda().eval()


@pytest.fixture(scope="module")
def model(params):
    return build(params)


def frames(T, B, H, W, seed=5):
    """T frames of B textured panoramas drifting by (1, 3) px per frame (horizontal wrap), on the device."""
    f0, _ = gc.synthetic_pair(B, H, W, seed=seed)
    return [torch.roll(f0, shifts=(t, 3 * t), dims=(2, 3)).cuda() for t in range(T)]


def epe(a, b):
    return float(po.epe(a.detach().cpu().float(), b.detach().cpu().float()).mean())


# ---- pf_forward_interpolate ------------------------------------------------------------------------------------------------
def field(kind, h, w, seed):
    g = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    if kind == "smooth":
        u = 3.0 * np.sin(x / w * 2 * np.pi + 0.3) + g.normal(0, 0.2, (h, w))
        v = 2.0 * np.cos(y / h * np.pi) + g.normal(0, 0.2, (h, w))
    elif kind == "large":           # displacements of a third of the frame: holes and pile-ups
        u = np.where(x < w / 2, 0.4 * w, -0.1 * w) + g.normal(0, 1.5, (h, w))
        v = np.where(y < h / 2, 0.25 * h, -0.05 * h) + g.normal(0, 1.5, (h, w))
    elif kind == "leaving":         # most points leave the frame
        u = (x - w / 2) * 0.8 + g.normal(0, 0.5, (h, w))
        v = (y - h / 2) * 0.8 + g.normal(0, 0.5, (h, w))
    elif kind == "invalid":
        u, v = np.full((h, w), 2.0 * w), np.full((h, w), -2.0 * h)
    else:
        raise ValueError(kind)
    return np.stack([u, v]).astype(np.float32)


@pytest.mark.parametrize("wrap", [False, True])
@pytest.mark.parametrize("kind", ["smooth", "large", "leaving", "invalid"])
@pytest.mark.parametrize("h,w", [(16, 32), (64, 128), (240, 480)])
def test_forward_interpolate_matches_brute_force(kind, h, w, wrap):
    """B = 2.  Every target at 16x32 and 64x128, 4096 sampled targets (and the first and last rows) at 240x480 -- 1/8 of
    1920x3840 -- against the float64 brute force: equal to its value bit for bit (same tie rule: lowest source index), which
    implies the issue's bar (exact where the nearest point is unique by > 1e-3 px, within 1e-3 px of the minimum elsewhere)."""
    from prior_flow_amd.evaluate import forward_interpolate
    flow = np.stack([field(kind, h, w, seed=s) for s in (11, 12)])
    out = forward_interpolate(torch.from_numpy(flow).cuda(), wrap=wrap).cpu().numpy()
    targets = None
    if h * w > 20000:
        g = np.random.default_rng(7)
        targets = np.unique(np.concatenate([g.choice(h * w, 4096, replace=False), np.arange(w), np.arange((h - 1) * w, h * w)]))
    for b in range(2):
        vals, idx, _, _ = fref.nearest(flow[b], wrap, targets)
        got = out[b].reshape(2, -1) if targets is None else out[b].reshape(2, -1)[:, targets]
        assert np.array_equal(got, vals), (b, int((got != vals).any(0).sum()))
        fref.check(out[b], flow[b], wrap, targets)
    if kind == "invalid":
        assert not out.any()


def test_forward_interpolate_shapes_and_capture():
    """[2,h,w] in, [2,h,w] out; the call is capturable (no host synchronisation) and a replay recomputes."""
    from prior_flow_amd._lib import load
    from prior_flow_amd.evaluate import forward_interpolate
    flow = torch.from_numpy(field("large", 64, 128, 3)).cuda()
    one = forward_interpolate(flow, wrap=True)
    assert tuple(one.shape) == (2, 64, 128) and one.dtype == torch.float32
    src = torch.zeros(1, 2, 64, 128, device="cuda")
    out = torch.zeros_like(src)
    scratch = torch.zeros(load().forward_interpolate_scratch_bytes(1, 64, 128) // 4, dtype=torch.int32, device="cuda")
    forward_interpolate(src, wrap=True, out=out, scratch=scratch)           # warm-up
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        forward_interpolate(src, wrap=True, out=out, scratch=scratch)
    src.copy_(flow[None])
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], one)


# ---- FlowStream -------------------------------------------------------------------------------------------------------------
def per_pair(model, fr, iters, inits=None):
    outs = []
    for t in range(1, len(fr)):
        init = None if inits is None else inits[t]
        outs.append(model(fr[t - 1], fr[t], iters=iters, init_flow=init, test_mode=True).clone())
    return outs


@pytest.mark.parametrize("B,H,W,iters", [(1, 128, 256, 4), (2, 128, 256, 4), (1, 512, 1024, 12), (2, 512, 1024, 12)])
def test_cold_stream_matches_per_pair_calls(model, B, H, W, iters):
    from prior_flow_amd.video import FlowStream
    fr = frames(5, B, H, W)
    with torch.no_grad():
        want = per_pair(model, fr, iters)
        s = FlowStream(model, iters=iters, warm_start=False)
        got = [s(f) for f in fr]
    assert got[0] is None and all(g is not None for g in got[1:])
    bitwise = all(torch.equal(g, w) for g, w in zip(got[1:], want))
    errs = [epe(g, w) for g, w in zip(got[1:], want)]
    print(f"cold stream B={B} {H}x{W}: bitwise equal to per-pair: {bitwise}; mean EPE per pair {errs}")
    assert max(errs) <= EPE_BATCH, errs


def test_warm_stream_matches_init_flow_calls(model):
    """Pair t >= 2 = model(f_t-1, f_t, init_flow=forward_interpolate(flow_low of pair t-1, wrap=True)); flow_low = the final
    coords1_A - coords0 of that call."""
    from prior_flow_amd.evaluate import forward_interpolate
    from prior_flow_amd.video import FlowStream
    B, H, W, iters = 2, 128, 256, 4
    fr = frames(5, B, H, W, seed=9)
    s = FlowStream(model, iters=iters, warm_start=True)
    with torch.no_grad():
        assert s(fr[0]) is None and s.flow_low is None
        prev_low = None
        for t in range(1, 5):
            got = s(fr[t])
            init = None if prev_low is None else forward_interpolate(prev_low, wrap=True)
            want = model(fr[t - 1], fr[t], iters=iters, init_flow=init, test_mode=True).clone()
            ws = model._ws[(B, H, W, str(fr[t].device))]
            low = (ws.c1a - ws.coords0).clone()
            assert epe(got, want) <= EPE_BATCH, (t, epe(got, want))
            assert float((s.flow_low - low).abs().max()) <= 1e-3, t
            if torch.equal(got, want):
                assert torch.equal(s.flow_low, low)
            prev_low = s.flow_low
        # the warm start changes the result (it is not silently cold)
        cold = model(fr[3], fr[4], iters=iters, test_mode=True)
        assert epe(got, cold) > 1e-4


@pytest.mark.parametrize("warm", [False, True])
def test_stream_graph_replay_equals_eager(model, warm):
    from prior_flow_amd.video import FlowStream
    fr = frames(5, 1, 128, 256, seed=3)
    with torch.no_grad():
        eager = [s for s in map(FlowStream(model, iters=4, warm_start=warm, use_graph=False), fr)]
        graph = [s for s in map(FlowStream(model, iters=4, warm_start=warm, use_graph=True), fr)]
    for e, g in zip(eager[1:], graph[1:]):
        assert torch.equal(e, g)


def test_stream_reuses_each_frame(model, monkeypatch):
    """After the first frame, a step launches fnet on 2B images and the input stage on one frame (the eager path runs the same
    launches the graph holds)."""
    from prior_flow_amd import _lib, engine
    from prior_flow_amd.video import FlowStream
    B = 2
    fr = frames(4, B, 128, 256)
    calls = {"fnet": [], "cnet": [], "frame": [], "pair": 0}
    run = engine.EncoderPlan.run

    def counted(plan, images, *a, **k):
        calls["fnet" if plan.kind == "instance" else "cnet"].append(images.shape[0])
        return run(plan, images, *a, **k)
    monkeypatch.setattr(engine.EncoderPlan, "run", counted)
    lib = _lib.load()
    prep_frame, prep_images = lib.prepare_frame, lib.prepare_images
    monkeypatch.setattr(lib, "prepare_frame", lambda img, *a: (calls["frame"].append(img.shape[0]), prep_frame(img, *a))[1])
    monkeypatch.setattr(lib, "prepare_images", lambda *a: (calls.__setitem__("pair", calls["pair"] + 1), prep_images(*a))[1])
    s = FlowStream(model, iters=2, warm_start=True, use_graph=False)
    with torch.no_grad():
        s(fr[0])
        for f in fr[1:]:
            for v in calls.values():
                if isinstance(v, list):
                    v.clear()
            s(f)
            assert calls["fnet"] == [2 * B] and calls["cnet"] == [2 * B], calls
            assert calls["frame"] == [B] and calls["pair"] == 0, calls


def test_stream_isolation_restart_and_edits(params):
    from prior_flow_amd.video import FlowStream
    m = build(params)
    fr = frames(4, 1, 128, 256, seed=21)
    other = frames(2, 1, 128, 256, seed=22)
    with torch.no_grad():
        ref = run_all(FlowStream(m, iters=3, warm_start=True), fr)
        # plain calls (graph replay and an eager warm-started one, same shape) between two steps change neither result
        plain0 = m(other[0], other[1], iters=3, test_mode=True).clone()
        s = FlowStream(m, iters=3, warm_start=True)
        got = [s(fr[0])]
        for f in fr[1:]:
            assert torch.equal(m(other[0], other[1], iters=3, test_mode=True), plain0)
            m(other[0], other[1], iters=3, init_flow=torch.ones(1, 2, 16, 32, device="cuda"), test_mode=True)
            got.append(s(f))
        assert torch.equal(m(other[0], other[1], iters=3, test_mode=True), plain0)
        for a, b in zip(ref[1:], got[1:]):
            assert torch.equal(a, b)
        # a shape switch restarts the stream; so does a mode switch
        s = FlowStream(m, iters=3, warm_start=False)
        assert s(fr[0]) is None and s(fr[1]) is not None
        assert s(frames(1, 1, 128, 512)[0]) is None
        assert s(frames(2, 1, 128, 512)[1]) is not None
        m.alternate_corr = True
        assert s(frames(3, 1, 128, 512)[2]) is None
        m.alternate_corr = None
        assert s(frames(1, 1, 128, 512)[0]) is None
        s.reset()
        assert s(fr[0]) is None and s.flow_low is None
        # in-place edits of fnet / cnet / update blocks are followed: the stream equals a fresh model's stream
        edits = {"fnet": lambda mm: mm.fnet.layer2[0].conv1.weight[:24, :, 1].add_(0.05),
                 "cnet": lambda mm: mm.cnet.conv2.bias.add_(0.1),
                 "update": lambda mm: mm.update_block.flow_head.conv2.bias.add_(0.2)}
        for name, edit in edits.items():
            s = FlowStream(m, iters=3, warm_start=False)
            s(fr[0])
            before = s(fr[1])
            edit(m)
            after = s(fr[2])
            fresh = build(params)
            fresh.load_state_dict(m.state_dict(), strict=True)
            want = fresh(fr[1], fr[2], iters=3, test_mode=True)
            assert epe(after, want) <= EPE_BATCH, (name, epe(after, want))
            assert before is not None


def run_all(stream, fr):
    return [stream(f) for f in fr]


@pytest.mark.parametrize("mode", ["mixed_precision", "alternate_corr", "both", "fp32", "wide"])
def test_stream_modes_match_their_per_pair_calls(params, mode):
    """Each inference mode's stream against its own per-pair calls (cold), and its warm stream against init_flow calls;
    'wide' is a 640x1280 stream (W/8 = 160)."""
    from prior_flow_amd import _lib
    from prior_flow_amd.evaluate import forward_interpolate
    from prior_flow_amd.video import FlowStream
    m = build(params, mixed_precision=mode in ("mixed_precision", "both"), alternate_corr=mode in ("alternate_corr", "both"))
    if mode == "fp32":
        m.precision = _lib.PREC_F32
    H, W = (640, 1280) if mode == "wide" else (128, 256)
    fr = frames(4, 1, H, W, seed=31)
    with torch.no_grad():
        want = per_pair(m, fr, 4)
        got = run_all(FlowStream(m, iters=4, warm_start=False), fr)
        errs = [epe(g, w) for g, w in zip(got[1:], want)]
        assert max(errs) <= EPE_BATCH, (mode, errs)
        s = FlowStream(m, iters=4, warm_start=True)
        s(fr[0])
        prev = None
        for t in range(1, 4):
            g = s(fr[t])
            init = None if prev is None else forward_interpolate(prev, wrap=True)
            w = m(fr[t - 1], fr[t], iters=4, init_flow=init, test_mode=True)
            assert epe(g, w) <= EPE_BATCH, (mode, t, epe(g, w))
            prev = s.flow_low


def test_stream_refuses_training_and_cpu(params):
    from prior_flow_amd._lib import PfError
    from prior_flow_amd.video import FlowStream
    m = build(params).train()
    fr = frames(1, 1, 128, 256)
    with pytest.raises(PfError):
        FlowStream(m, iters=2)(fr[0])
    with pytest.raises(PfError):
        FlowStream(build(params), iters=2)(fr[0].cpu())


def test_evicting_a_batch_keeps_the_encoder_buffers_of_twice_that_batch(params):
    """cnet of a B = 2 pair and fnet of a B = 1 pair (and fnet of a B = 2 stream) all run 4 images at one size.  Evicting the
    B = 1 workspace must not drop cnet's buffers of the resident B = 2 workspace: its captured graph replays into them."""
    m = build(params)
    m.WS_KEEP = 2
    one, two = frames(2, 1, 128, 256), frames(2, 2, 128, 256)
    with torch.no_grad():
        m(one[0], one[1], iters=2, test_mode=True)
        first = m(two[0], two[1], iters=2, test_mode=True).clone()
        m(*frames(2, 1, 128, 512), iters=2, test_mode=True)          # evicts (1, 128, 256)
        assert (1, 128, 256, "cuda:0") not in m._ws and (2, 128, 256, "cuda:0") in m._ws
        cplan = m._encoder_plans()[0]
        assert any(k[-3:] == (4, 128, 256) for k in cplan._bufs_by_key), list(cplan._bufs_by_key)
        assert torch.equal(m(two[0], two[1], iters=2, test_mode=True), first)
