"""Push-pull hole filling on an MI355X: pf_fill_pushpull and the level-by-level entry points on the device
against the host emulation of the same functions bit for bit (maps at two alignments, outputs pre-filled, scratch poisoned), fused
against level by level, run against run, in place against out of place, the exact properties and the quality scene on the device,
and the Python layer: FrameInterpolator(fill="pushpull") eager and captured behind a bidirectional FlowStream, the Reprojector
option, the refusals.  Run with ``-m gpu``."""
import argparse

import numpy as np
import pytest
import torch

import fill_cases as fc
import fill_ref as fr
import golden_cases as gc

pytestmark = pytest.mark.gpu
DEV = "cuda"
same = fc.same


@pytest.fixture(scope="module")
def emu():
    return fc.emu()


@pytest.fixture(scope="module")
def lib():
    from prior_flow_amd._lib import load
    return load()


@pytest.mark.parametrize("kind", fc.FAMILIES)
def test_device_matches_the_emulation(lib, emu, kind):
    """Every shape of the sweep, twice -- maps as allocated and maps one element into a larger buffer --, out pre-filled with NaN,
    empty with 0xFF, scratch poisoned with NaN / +-1e30 before each call: out and empty of the fused form and of the level-by-level
    form on the device are the emulation's bits."""
    n = 0
    for k, (B, C, H, W) in fc.sweep():
        if k != kind:
            continue
        src, hole, weight = fc.inputs(kind, B, C, H, W)
        want, we, _ = fc.run(emu, src, hole, weight)
        for offset in (0, 1):
            got, ge, _ = fc.run(lib, src, hole, weight, DEV, "fused", offset)
            assert same(got, want) and np.array_equal(ge, we), (kind, B, C, H, W, offset, "fused")
            got, ge, f = fc.run(lib, src, hole, weight, DEV, "levels", offset)
            assert same(got, want) and np.array_equal(ge, we), (kind, B, C, H, W, offset, "levels")
        # the device's pyramid, through the level entry points, is the restatement's
        r = fr.fill(src[0], hole[0], None if weight is None else weight[0])
        for l in range(1, fr.levels(H, W) + 1):
            assert same(f.levels[l - 1][0][0].cpu().numpy(), r["filled"][l]) and same(f.levels[l - 1][1][0].cpu().numpy(), r["pulled"][l][1])
        n += 1
    print(f"{kind}: {n} shapes, two alignments, two forms")


def test_levels_between_the_tile_kernels_and_the_apex(lib, emu):
    """300x2300 at C = 4: the levels above the fifth do not fit the apex kernel's LDS, one pull and one push run level by level in
    the fused call.  The emulation's bits, and those of the level-by-level form."""
    B, C, H, W = fc.BIG
    assert fc.plan(C, H, W)[1:] == (5, 6)
    src, hole, weight = fc.inputs("bern95", B, C, H, W)
    want, we, _ = fc.run(emu, src, hole, weight)
    got, ge, f = fc.run(lib, src, hole, weight, DEV, "fused")
    assert same(got, want) and np.array_equal(ge, we)
    again, _, _ = fc.run(lib, src, hole, weight, DEV, "levels", filler=f)
    assert same(again, want)


def test_the_three_stages_in_order_are_the_fused_call(lib, emu):
    """pf_fill_stage 0, 1, 2 on a poisoned scratch give pf_fill_pushpull's bits; a stage refuses what the whole call refuses."""
    from prior_flow_amd._lib import PfError
    for handle, dev in ((lib, DEV), (emu, "cpu")):
        for B, C, H, W in ((2, 3, 33, 70), (1, 1, 1, 1)):
            src, hole, weight = fc.inputs("soft", B, C, H, W)
            want, we, f = fc.run(handle, src, hole, weight, dev)
            fc.poison_scratch(f)
            s, h, w = fc._t(src, dev), fc._t(hole, dev), fc._t(weight, dev)
            out = torch.full_like(s, float("nan"))
            for stage in (0, 1, 2):
                handle.fill_pushpull(s, h, w, out, f.empty, f.scratch, stage=stage)
            assert same(out.cpu().numpy(), want) and np.array_equal(f.empty.cpu().numpy(), we)
            with pytest.raises(PfError):
                handle.fill_pushpull(s, h, w, out, f.empty, f.scratch, stage=3)


def test_same_bits_on_every_run_in_place_and_at_512x1024(lib):
    """At the flagship size 512x1024 (C = 3, Bernoulli 0.5): two runs of the fused form, the level-by-level form and the fill in
    place (out is src) give the same bits; valid pixels keep theirs."""
    B, C, H, W = 1, 3, 512, 1024
    src, hole, _ = fc.inputs("bern50", B, C, H, W)
    a, ea, f = fc.run(lib, src, hole, None, DEV, "fused")
    b, eb, _ = fc.run(lib, src, hole, None, DEV, "fused", filler=f)
    c, _, _ = fc.run(lib, src, hole, None, DEV, "levels", filler=f)
    d, _, _ = fc.run(lib, src, hole, None, DEV, "fused", in_place=True, filler=f)
    assert same(a, b) and same(a, c) and same(a, d) and np.array_equal(ea, eb) and not ea.any()
    keep = np.broadcast_to(hole[:, None] == 0, src.shape)
    assert np.array_equal(fc.bits(a)[keep], fc.bits(src)[keep]) and np.isfinite(a).all()
    for kind, shape in (("soft", (2, 4, 33, 70)), ("seam", (3, 2, 24, 48))):
        src, hole, weight = fc.inputs(kind, *shape)
        a, _, _ = fc.run(lib, src, hole, weight, DEV, "fused")
        b, _, _ = fc.run(lib, src, hole, weight, DEV, "fused", in_place=True)
        assert same(a, b), kind


@pytest.mark.parametrize("check", fc.EXACT_CHECKS, ids=lambda c: c.__name__)
def test_property_on_the_device(lib, check):
    check(fc.filler_fn(lib, DEV, "fused"))


def test_quality_scene_on_the_device(lib):
    """The quality scene at 32x64 and 64x128: the device's rms error inside the holes is the float64 restatement's within the bound
    on |fp32 - float64| (an rms of differences is at most their maximum), and below a quarter of the mean fill's."""
    for H, W in ((32, 64), (64, 128)):
        got, mean_fill, band = fc.quality_figures(fc.filler_fn(lib, DEV), H, W)
        want = fc.quality_figures(fc.ref_fn(dtype=np.float64), H, W)
        img, hole, _ = fc.quality_scene(H, W)
        tol = fr.bound(fr.levels(H, W), float(np.abs(img.astype(np.float32)).max()), False)
        print(f"{H}x{W}: rms in holes {got:.4f} (float64 restatement {want[0]:.4f}, bound {tol:.2e}), valid mean {mean_fill:.2f}, seam band {band:.3f}")
        assert abs(got - want[0]) <= tol and abs(band - want[2]) <= tol and got < 0.25 * mean_fill


def test_python_layer_on_the_device(lib):
    """HoleFiller and fill_holes on device tensors; the Reprojector option equals a fill by hand; every refusal launches nothing
    and leaves the buffers as they were."""
    from prior_flow_amd._lib import PfError
    from prior_flow_amd.inpaint import HoleFiller, fill_holes
    from prior_flow_amd.interp import FrameInterpolator
    from prior_flow_amd.reproject import Reprojector
    B, C, H, W = 2, 3, 24, 48
    src, hole, weight = (fc._t(a, DEV) for a in fc.inputs("soft", B, C, H, W))
    f = HoleFiller(B, C, H, W, DEV)
    out, empty = f.fill(src, hole, weight)
    once = fill_holes(src, hole, weight)
    lv, _ = HoleFiller(B, C, H, W, DEV).fill_levels(src, hole, weight)
    assert torch.equal(out, once[0]) and torch.equal(out, lv) and torch.equal(empty, once[1]) and not empty.any()
    rng = np.random.default_rng(1)
    d0 = fc._t(np.exp2(rng.uniform(-3, 1, (B, H, W))).astype(np.float32), DEV)
    w0 = fc._t((rng.random((B, H, W)) > 0.2).astype(np.float32), DEV)
    R = torch.eye(3, device=DEV).repeat(B, 1, 1).contiguous()
    T = torch.tensor([[0.3, 0.1, -0.2]] * B, device=DEV)
    rp, plain = Reprojector(B, C, H, W, DEV, fill=True), Reprojector(B, C, H, W, DEV)
    res, ref = rp.run(src, d0, w0, R, T), plain.run(src, d0, w0, R, T)
    assert all(torch.equal(x, y) for x, y in zip(res, ref)) and bool(res[3].any())
    hf, _ = HoleFiller(B, C, H, W, DEV).fill(res[0], res[3])
    hd, _ = HoleFiller(B, 1, H, W, DEV).fill(res[1].view(B, 1, H, W), res[3], res[2])
    assert torch.equal(rp.filled, hf) and torch.equal(rp.filled_inv_depth, hd.view(B, H, W))
    first = out.clone()
    f.scratch.fill_(3.5); f.out.fill_(-2.0); f.empty.fill_(9)
    both = torch.zeros(2 * B * C * H * W, device=DEV)
    part, shifted = both[:B * C * H * W].view(B, C, H, W), both[4:4 + B * C * H * W].view(B, C, H, W)
    for bad in (lambda: f.fill(src.cpu(), hole), lambda: f.fill(src, hole.cpu()), lambda: f.fill(src, hole, weight.cpu()),
                lambda: fill_holes(src.cpu(), hole.cpu()), lambda: HoleFiller(B, C, H, W, "cpu"),
                lambda: f.fill(src.double(), hole), lambda: f.fill(src, hole.float()), lambda: f.fill(src[:, :2], hole),
                lambda: f.fill(src[:, :, :, ::2], hole[:, :, ::2]), lambda: f.fill(src, hole, out=src.cpu()),
                lambda: f.fill(src.transpose(2, 3).contiguous().transpose(2, 3), hole),
                lambda: f.fill(part, hole, out=shifted), lambda: f.fill_levels(part, hole, out=shifted),
                lambda: f.fill(src, hole, weight, out=weight.view(B, 1, H, W).expand(B, C, H, W)),
                lambda: f.fill(src, hole, f.w0), lambda: f.fill(f.out, hole, out=f.out[:, :, :, :W // 2]),
                lambda: FrameInterpolator(B, C, H, W, DEV, fill="inpaint"), lambda: Reprojector(B, C, H, W, DEV, fill=1)):
        with pytest.raises(PfError):
            bad()
    torch.cuda.synchronize()
    assert bool((f.scratch == 3.5).all()) and bool((f.out == -2.0).all()) and bool((f.empty == 9).all()) and not both.any()
    s = src.clone()
    got, _ = f.fill(s, hole, weight, out=s)
    assert got is s and torch.equal(s, first)


def test_interpolator_pushpull_behind_the_stream_eager_and_captured():
    """Three frames at 128x256 on the tiny model, iters = 2, through a cold bidirectional FlowStream: FrameInterpolator(fill=
    "pushpull").from_bidirectional equals fill="none" followed by a fill by hand, allocates nothing after its first call, and as a
    captured graph replayed on copied-in inputs over a poisoned output and poisoned scratch it gives the eager bits."""
    from prior_flow_amd.inpaint import HoleFiller
    from prior_flow_amd.interp import FrameInterpolator
    from prior_flow_amd.modules import state_dict_shapes
    from prior_flow_amd.prior_raft import PriOr_RAFT
    from prior_flow_amd.video import BidirectionalFlow, FlowStream
    B, H, W = 1, 128, 256
    m = PriOr_RAFT(argparse.Namespace(mixed_precision=False, dropout=0.0, alternate_corr=False))
    m.load_state_dict(gc.det_state_dict(state_dict_shapes()), strict=True)
    m = m.cuda().eval()
    f0, _ = gc.synthetic_pair(B, H, W, seed=5)
    frames = [torch.roll(f0, shifts=(t, 3 * t), dims=(2, 3)).cuda().contiguous() for t in range(3)]
    stream = FlowStream(m, iters=2, bidirectional=True, occlusion="plane")
    fi, none = FrameInterpolator(B, 3, H, W, DEV, fill="pushpull"), FrameInterpolator(B, 3, H, W, DEV, fill="none")
    hand = HoleFiller(B, 3, H, W, DEV)
    results, eager = [], []
    with torch.no_grad():
        assert stream(frames[0]) is None
        for i in (1, 2):
            r = BidirectionalFlow(*[t.clone() for t in stream(frames[i])])
            if i == 2:
                torch.cuda.synchronize()
                n0 = torch.cuda.memory_stats()["allocation.all.allocated"]
            out, hole = fi.from_bidirectional(r, frames[i - 1], frames[i], 0.5, use_occlusion=True)
            if i == 2:
                assert torch.cuda.memory_stats()["allocation.all.allocated"] == n0, "a filled interpolation allocated device memory"
            raw, rh = none.from_bidirectional(r, frames[i - 1], frames[i], 0.5, use_occlusion=True)
            want, _ = hand.fill(raw, rh)
            assert torch.equal(out, want) and torch.equal(hole, rh) and bool(torch.isfinite(out).all())
            assert not raw[:, 0][rh != 0].any()
            results.append(r)
            eager.append((out.clone(), hole.clone()))
        print(f"[fill] behind the stream: {float((eager[1][1] != 0).float().mean()):.2%} of the interpolated frame are holes")
        cap = FrameInterpolator(B, 3, H, W, DEV, fill="pushpull")
        static = BidirectionalFlow(*[torch.zeros_like(t) for t in results[0]])
        a, b = torch.zeros_like(frames[0]), torch.zeros_like(frames[1])
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            cap.from_bidirectional(static, a, b, 0.5, use_occlusion=True)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            cap.from_bidirectional(static, a, b, 0.5, use_occlusion=True)
        for i, (r, want) in enumerate(zip(results, eager)):
            for dst, src in zip(static, r):
                dst.copy_(src)
            a.copy_(frames[i])
            b.copy_(frames[i + 1])
            cap.out.fill_(float("nan"))
            fc.poison_scratch(cap.filler)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(cap.out, want[0]) and torch.equal(cap.hole, want[1]) and not cap.acc.any()
