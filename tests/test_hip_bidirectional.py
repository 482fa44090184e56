"""Bidirectional video flow on an MI355X: pf_fb_check on the device against the float64 restatement (tests/fb_check_ref.py) and
the host emulation, and FlowStream(bidirectional=True) (prior-flow_amd/video.py) against the unchanged per-pair model(...) calls
in both directions -- cold, warm-started, graph against eager, the frame cache's reuse (cnet included), masks, modes, restarts,
isolation and weight edits.  Run with ``-m gpu``.

Bitwise against the emulation library: the round trip (`residual`) under both metrics and the `plane` mask -- additions,
multiplications, floor and one fma, compiled without contraction on both sides, like the project's other samplers.  The
`sphere` mask goes through sinf / cosf / asinf, which the device's math library and the host's round differently: it is held to
the float64 bounds (every decided pixel right), and the number of pixels where it differs from the emulation is printed."""
import argparse

import numpy as np
import pytest
import torch

import fb_check_ref as fb
import golden_cases as gc
import priorflow_oracle as po
from test_fb_check_host import check_case, emu, run  # noqa: F401  (emu: the emulation library's fixture)
from test_hip_stream import EPE_BATCH                # the project's batch-independence bar (mean EPE), reused

pytestmark = pytest.mark.gpu


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


def same(a, b):
    """Two stream results (or None) equal bit for bit, masks and residuals included."""
    if a is None or b is None:
        return a is None and b is None
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


# ---- pf_fb_check ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["plane", "sphere"])
@pytest.mark.parametrize("H,W", [(64, 128), (128, 256), (512, 1024)])
@pytest.mark.parametrize("kind", fb.KINDS)
def test_fb_check_matches_float64_and_the_emulation(emu, kind, H, W, metric):  # noqa: F811
    from prior_flow_amd._lib import load
    figures = check_case(load(), kind, H, W, metric, device="cuda")
    assert all(0.0 < f["occluded"] < 1.0 for f in figures)
    fw, bw = fb.batch(kind, H, W)
    dev, host = run(load(), fw, bw, metric, device="cuda"), run(emu, fw, bw, metric)
    differ = [int((d != h).sum()) for d, h in zip(dev, host)]
    print(f"{kind} {H}x{W} {metric}: elements differing from the emulation (occ_fw, occ_bw, res_fw, res_bw): {differ}")
    assert differ[2] == 0 and differ[3] == 0
    if metric == "plane":
        assert differ[0] == 0 and differ[1] == 0


def test_fb_check_unaligned_width_takes_the_element_form(emu):  # noqa: F811
    """W % 4 != 0: one pixel per thread; same statement, same bits as the emulation."""
    from prior_flow_amd._lib import load
    fw, bw = fb.batch("seam", 64, 126)
    for metric in ("plane", "sphere"):
        dev, host = run(load(), fw, bw, metric, device="cuda"), run(emu, fw, bw, metric)
        for b in range(2):
            fb.check(dev[0][b], dev[2][b], fb.reference(fw[b], bw[b], metric), f"seam 64x126 {metric} image {b} forward")
            fb.check(dev[1][b], dev[3][b], fb.reference(bw[b], fw[b], metric), f"seam 64x126 {metric} image {b} backward")
        assert np.array_equal(dev[2], host[2]) and np.array_equal(dev[3], host[3])


def test_fb_check_is_deterministic_capturable_and_refuses_cpu_tensors():
    from prior_flow_amd._lib import PfError
    from prior_flow_amd.video import forward_backward_check
    fw, bw = (torch.from_numpy(a).cuda() for a in fb.batch("poles", 128, 256))
    one = forward_backward_check(fw, bw, metric="sphere")
    two = forward_backward_check(fw, bw, metric="sphere")
    assert one[0].dtype == torch.uint8 and tuple(one[0].shape) == (2, 128, 256) and tuple(one[2].shape) == (2, 2, 128, 256)
    assert all(torch.equal(a, b) for a, b in zip(one, two))
    src = (torch.zeros_like(fw), torch.zeros_like(bw))
    out = tuple(torch.zeros_like(t) for t in one)
    forward_backward_check(*src, metric="sphere", out=out)                  # warm-up
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        forward_backward_check(*src, metric="sphere", out=out)
    src[0].copy_(fw)
    src[1].copy_(bw)
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(one, out))
    with pytest.raises(PfError):
        forward_backward_check(fw.cpu(), bw.cpu())
    with pytest.raises(PfError):
        forward_backward_check(fw, bw, metric="cube")


# ---- FlowStream(bidirectional=True) -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,iters", [(1, 128, 256, 4), (2, 128, 256, 4), (1, 512, 1024, 12), (2, 512, 1024, 12)])
def test_cold_bidirectional_stream_matches_per_pair_calls(model, B, H, W, iters):
    """The yardstick is the unchanged per-pair call, in each direction."""
    from prior_flow_amd.video import FlowStream
    fr = frames(5, B, H, W)
    with torch.no_grad():
        s = FlowStream(model, iters=iters, warm_start=False, bidirectional=True)
        got = [s(f) for f in fr]
        assert got[0] is None
        errs, bitwise = [], True
        for t in range(1, 5):
            fwd = model(fr[t - 1], fr[t], iters=iters, test_mode=True).clone()
            bwd = model(fr[t], fr[t - 1], iters=iters, test_mode=True).clone()
            assert got[t].occ_forward is None and got[t].residual_backward is None
            assert tuple(got[t].forward.shape) == tuple(got[t].backward.shape) == (B, 2, H, W)
            errs.append((epe(got[t].forward, fwd), epe(got[t].backward, bwd)))
            bitwise = bitwise and torch.equal(got[t].forward, fwd) and torch.equal(got[t].backward, bwd)
    print(f"cold bidirectional stream B={B} {H}x{W}: bitwise equal to the per-pair calls: {bitwise}; mean EPE (forward, backward) {errs}")
    assert max(max(e) for e in errs) <= EPE_BATCH, errs


def test_warm_bidirectional_stream_matches_init_flow_calls(model):
    """Forward pair t: init_flow = forward_interpolate(flow_low of pair t-1, wrap=True); backward pair t:
    -forward_interpolate(-flow_low_backward of pair t-1, wrap=True).  And neither is silently cold."""
    from prior_flow_amd.evaluate import forward_interpolate
    from prior_flow_amd.video import FlowStream
    B, H, W, iters = 2, 128, 256, 4
    fr = frames(6, B, H, W, seed=9)
    s = FlowStream(model, iters=iters, warm_start=True, bidirectional=True)
    with torch.no_grad():
        assert s(fr[0]) is None and s.flow_low is None and s.flow_low_backward is None
        low_f = low_b = None
        for t in range(1, 6):
            got = s(fr[t])
            init_f = None if low_f is None else forward_interpolate(low_f, wrap=True)
            init_b = None if low_b is None else -forward_interpolate(-low_b, wrap=True)
            want_f = model(fr[t - 1], fr[t], iters=iters, init_flow=init_f, test_mode=True).clone()
            ws = model._ws[(B, H, W, str(fr[t].device))]
            wlow_f = (ws.c1a - ws.coords0).clone()
            want_b = model(fr[t], fr[t - 1], iters=iters, init_flow=init_b, test_mode=True).clone()
            wlow_b = (ws.c1a - ws.coords0).clone()
            e = (epe(got.forward, want_f), epe(got.backward, want_b))
            print(f"warm pair {t}: mean EPE (forward, backward) {e}")
            assert max(e) <= EPE_BATCH, (t, e)
            low_f, low_b = s.flow_low, s.flow_low_backward
            assert float((low_f - wlow_f).abs().max()) <= 1e-3 and float((low_b - wlow_b).abs().max()) <= 1e-3, t
        cold_f = model(fr[4], fr[5], iters=iters, test_mode=True).clone()
        cold_b = model(fr[5], fr[4], iters=iters, test_mode=True).clone()
        assert epe(got.forward, cold_f) > 1e-4 and epe(got.backward, cold_b) > 1e-4


def test_bidirectional_stream_reuses_each_frame(model, monkeypatch):
    """After the first frame a step launches fnet on 2B images, cnet on 2B images (the new frame's two views only) and the
    input stage on one frame; the eager path runs the launches the graph holds."""
    from prior_flow_amd import _lib, engine
    from prior_flow_amd.video import FlowStream
    B = 2
    fr = frames(5, B, 128, 256)
    calls = {"fnet": [], "cnet": [], "frame": [], "pair": 0}
    run_plan = engine.EncoderPlan.run

    def counted(plan, images, *a, **k):
        calls["fnet" if plan.kind == "instance" else "cnet"].append(images.shape[0])
        return run_plan(plan, images, *a, **k)
    monkeypatch.setattr(engine.EncoderPlan, "run", counted)
    lib = _lib.load()
    prep_frame, prep_images = lib.prepare_frame, lib.prepare_images
    monkeypatch.setattr(lib, "prepare_frame", lambda img, *a: (calls["frame"].append(img.shape[0]), prep_frame(img, *a))[1])
    monkeypatch.setattr(lib, "prepare_images", lambda *a: (calls.__setitem__("pair", calls["pair"] + 1), prep_images(*a))[1])
    s = FlowStream(model, iters=2, warm_start=True, use_graph=False, bidirectional=True, occlusion="sphere")
    with torch.no_grad():
        s(fr[0])
        assert calls["fnet"] == [2 * B] and calls["cnet"] == [2 * B] and calls["frame"] == [B], calls
        for f in fr[1:]:
            for v in calls.values():
                if isinstance(v, list):
                    v.clear()
            assert s(f) is not None
            assert calls["fnet"] == [2 * B] and calls["cnet"] == [2 * B], calls
            assert calls["frame"] == [B] and calls["pair"] == 0, calls


@pytest.mark.parametrize("warm", [False, True])
def test_bidirectional_graph_replay_equals_eager(model, warm):
    """9 frames: a parity's graph is captured at its first step in a mode (cold: frames 1, 2; warm: frames 2, 3 after the cold
    frame 1), so both parities are replayed at least twice."""
    from prior_flow_amd.video import FlowStream
    fr = frames(9, 1, 128, 256, seed=3)
    with torch.no_grad():
        eager = [r for r in map(FlowStream(model, iters=3, warm_start=warm, use_graph=False, bidirectional=True, occlusion="sphere"), fr)]
        gs = FlowStream(model, iters=3, warm_start=warm, use_graph=True, bidirectional=True, occlusion="sphere")
        graph = [r for r in map(gs, fr)]
    assert sorted(k[2] for k in gs._st.graphs) == ([0, 1] if not warm else [0, 1, 1])
    assert eager[0] is None and graph[0] is None
    for t, (e, g) in enumerate(zip(eager[1:], graph[1:]), 1):
        assert same(e, g), t


@pytest.mark.parametrize("metric", ["sphere", "plane"])
def test_stream_masks_are_the_check_on_its_own_flows(model, metric):
    from prior_flow_amd.video import FlowStream, forward_backward_check, run_sequence
    fr = frames(4, 2, 128, 256, seed=13)
    with torch.no_grad():
        res = run_sequence(model, fr, iters=3, warm_start=True, bidirectional=True, occlusion=metric)
        assert len(res) == 3
        for r in res:
            want = forward_backward_check(r.forward, r.backward, metric=metric)
            assert r.occ_forward.dtype == torch.uint8 and tuple(r.occ_forward.shape) == (2, 128, 256)
            assert all(torch.equal(a, b) for a, b in zip(r[2:], want))
        plain = run_sequence(model, fr, iters=3, warm_start=True, bidirectional=True)
        assert all(p.occ_forward is None and torch.equal(p.forward, r.forward) and torch.equal(p.backward, r.backward)
                   for p, r in zip(plain, res))
        one_way = run_sequence(model, fr, iters=3, warm_start=True)          # the default path is what it was: tensors
        assert all(isinstance(f, torch.Tensor) for f in one_way)
        assert isinstance(FlowStream(model, bidirectional=True).bidirectional, bool)


@pytest.mark.parametrize("mode", ["mixed_precision", "alternate_corr", "fp32"])
def test_bidirectional_modes_match_their_per_pair_calls(params, mode):
    """Each inference mode's bidirectional stream against its own per-pair calls, cold and warm."""
    from prior_flow_amd import _lib
    from prior_flow_amd.evaluate import forward_interpolate
    from prior_flow_amd.video import FlowStream
    m = build(params, mixed_precision=mode == "mixed_precision", alternate_corr=mode == "alternate_corr")
    if mode == "fp32":
        m.precision = _lib.PREC_F32
    fr = frames(4, 1, 128, 256, seed=31)
    with torch.no_grad():
        got = [r for r in map(FlowStream(m, iters=4, warm_start=False, bidirectional=True), fr)]
        for t in range(1, 4):
            e = (epe(got[t].forward, m(fr[t - 1], fr[t], iters=4, test_mode=True)),
                 epe(got[t].backward, m(fr[t], fr[t - 1], iters=4, test_mode=True)))
            assert max(e) <= EPE_BATCH, (mode, "cold", t, e)
        s = FlowStream(m, iters=4, warm_start=True, bidirectional=True)
        s(fr[0])
        low_f = low_b = None
        for t in range(1, 4):
            g = s(fr[t])
            init_f = None if low_f is None else forward_interpolate(low_f, wrap=True)
            init_b = None if low_b is None else -forward_interpolate(-low_b, wrap=True)
            e = (epe(g.forward, m(fr[t - 1], fr[t], iters=4, init_flow=init_f, test_mode=True)),
                 epe(g.backward, m(fr[t], fr[t - 1], iters=4, init_flow=init_b, test_mode=True)))
            assert max(e) <= EPE_BATCH, (mode, "warm", t, e)
            low_f, low_b = s.flow_low, s.flow_low_backward


def test_bidirectional_isolation_restart_and_edits(params):
    from prior_flow_amd.video import FlowStream
    m = build(params)
    fr = frames(5, 1, 128, 256, seed=21)
    other = frames(3, 1, 128, 256, seed=22)
    bi = lambda **kw: FlowStream(m, iters=3, bidirectional=True, occlusion="sphere", **kw)     # noqa: E731
    with torch.no_grad():
        ref = [r for r in map(bi(warm_start=True), fr)]
        # a plain call (graph replay and an eager warm-started one) and a one-direction stream between two steps disturb nothing
        plain0 = m(other[0], other[1], iters=3, test_mode=True).clone()
        one_way = FlowStream(m, iters=3, warm_start=True)
        one_ref = [f for f in map(FlowStream(m, iters=3, warm_start=True), other)]
        s = bi(warm_start=True)
        got, one_got = [], []
        for t, f in enumerate(fr):
            got.append(s(f))
            assert torch.equal(m(other[0], other[1], iters=3, test_mode=True), plain0)
            m(other[0], other[1], iters=3, init_flow=torch.ones(1, 2, 16, 32, device="cuda"), test_mode=True)
            if t < len(other):
                one_got.append(one_way(other[t]))
        assert all(same(a, b) for a, b in zip(ref, got))
        assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(one_ref, one_got))
        # a shape switch restarts the stream; so do a mode switch and reset()
        s = bi(warm_start=False)
        assert s(fr[0]) is None and s(fr[1]) is not None
        assert s(frames(1, 1, 128, 512)[0]) is None
        assert s(frames(2, 1, 128, 512)[1]) is not None
        m.alternate_corr = True
        assert s(frames(3, 1, 128, 512)[2]) is None
        m.alternate_corr = None
        assert s(frames(1, 1, 128, 512)[0]) is None
        s.reset()
        assert s(fr[0]) is None and s.flow_low is None and s.flow_low_backward is None
        assert same(s(fr[1]), ref[1])                    # the first pair after a restart is the cold first pair
        # in-place edits are followed, cnet's included (the cached frame's cnet outputs are part of the cache now): the pair
        # after the edit equals a fresh model's per-pair calls, at either parity of the cached frame
        edits = {"fnet": lambda mm: mm.fnet.layer2[0].conv1.weight[:24, :, 1].add_(0.05),
                 "cnet": lambda mm: mm.cnet.conv2.bias.add_(0.1),
                 "cnet, odd frame": lambda mm: mm.cnet.conv2.bias.add_(0.1),
                 "update": lambda mm: mm.update_block.flow_head.conv2.bias.add_(0.2)}
        for name, edit in edits.items():
            k = 2 if "odd" in name else 1            # the frame cached when the edit happens
            s = bi(warm_start=False)
            before = [s(f) for f in fr[:k + 1]][-1]
            edit(m)
            after = s(fr[k + 1])
            fresh = build(params)
            fresh.load_state_dict(m.state_dict(), strict=True)
            e = (epe(after.forward, fresh(fr[k], fr[k + 1], iters=3, test_mode=True)),
                 epe(after.backward, fresh(fr[k + 1], fr[k], iters=3, test_mode=True)))
            assert max(e) <= EPE_BATCH, (name, e)
            assert before is not None


def test_bidirectional_stream_refuses_training_and_cpu(params):
    from prior_flow_amd._lib import PfError
    from prior_flow_amd.video import FlowStream
    fr = frames(1, 1, 128, 256)
    with pytest.raises(PfError):
        FlowStream(build(params).train(), iters=2, bidirectional=True)(fr[0])
    with pytest.raises(PfError):
        FlowStream(build(params), iters=2, bidirectional=True)(fr[0].cpu())
