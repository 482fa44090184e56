"""Forward softmax splatting on an MI355X: pf_splat_accumulate and pf_splat_resolve (both launch forms)
on the device against the float64 restatement (tests/splat_ref.py) and, where no expf is evaluated, bit for bit against the host
emulation of the same functions; reproducibility under repeated calls and reordered jobs; the Python layer
(prior_flow_amd.interp), eager and captured, behind a bidirectional FlowStream.  Run with ``-m gpu``."""
import argparse

import numpy as np
import pytest
import torch

import golden_cases as gc
import splat_cases as sc
import splat_ref as sr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def emu():
    return sc.emu()


@pytest.fixture(scope="module")
def lib():
    from prior_flow_amd._lib import load
    return load()


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("kind", sr.FAMILIES)
def test_device_matches_float64_and_the_emulation(lib, emu, kind):
    """Every case of the sweep: the device holds the float64 bounds; 17x37 takes resolve's element form, 24x48 and 64x128 four
    pixels per thread.  At alpha = 0 there is no metric and no expf: out, the hole byte and the raw sums before resolve are the
    emulation's bits.  At alpha > 0 the number of differing values is printed, not asserted (expf is the device's)."""
    worst, n, differ, values = 0.0, 0, 0, 0
    for case in sr.sweep():
        if case[0] != kind:
            continue
        refs = {}
        out, hole, raw, figs = sc.check_case(lib, *case, device="cuda", refs=refs)
        h = sc.check_case(emu, *case, refs=refs)
        worst = max([worst] + [f["err_over_tol"] for f in figs])
        n += 1
        if case[3] == 0.0:
            assert same((out, hole, raw), h[:3]), case
        else:
            differ += int((bits(out) != bits(h[0])).sum()) + int((raw != h[2]).sum())
            values += out.size + raw.size
    print(f"{kind}: {n} cases, worst err / bound {worst:.4f}; alpha > 0: {differ} of {values} values differ from the emulation")


@pytest.mark.parametrize("kind", sr.DEVICE_FAMILIES)
def test_window_cases_match_float64_and_the_emulation(lib, emu, kind):
    """sc.DEVICE_PATHS: the code of pf_splat_acc_kernel that no other file holds -- where a window is placed (and that it is placed
    at the tile when the centre pixel lands nowhere), its columns modulo a width below, at and above its own, the
    window-or-direct choice of a tap, the flush -- at four tile columns, at 64 < W <= 80 and with blockIdx.z > 0 beside tx0 > 0.
    Every case holds the float64 bounds; at alpha = 0 out, the hole byte and the raw sums are the emulation's bits (the
    emulation adds every tap directly: where an add is made must not change a bit); a second run and the jobs reversed give the
    first run's bits; the sums are all-zero afterwards.  `centre_far` (a centre that is splatted but lands beyond 2^28) is
    beyond the reference and is held to the emulation's bits.  Prints the paths each case reaches (tests/launch_paths.py)."""
    cases = [c for c in sc.DEVICE_PATHS if c[0] == kind] + ([sr.CENTRE_FAR] if kind == "centre_bad" else [])
    worst, differ, values, union = 0.0, 0, 0, set()
    for case in cases:
        _, (B, H, W), t, alpha, C, njobs = case
        paths = sc.reached(case)
        union |= paths
        print(f"{case}: reaches {sorted(paths)}")
        if case[0] == "centre_far":
            jobs = sc.case_inputs(*case)
            out, hole, raw, after = sc.run(lib, jobs, alpha, "cuda")
            h = sc.run(emu, jobs, alpha)
            assert not after.any()
        else:
            refs = {}
            out, hole, raw, figs = sc.check_case(lib, *case, device="cuda", refs=refs)
            h = sc.check_case(emu, *case, refs=refs)
            worst = max([worst] + [f["err_over_tol"] for f in figs])
        if alpha == 0.0:
            assert same((out, hole, raw), h[:3]), case
        else:
            differ += int((bits(out) != bits(h[0])).sum()) + int((raw != h[2]).sum())
            values += out.size + raw.size
        jobs = sc.case_inputs(*case)
        fill = (jobs[0]["src"], jobs[1]["src"]) if njobs == 2 and case[0] != "centre_far" else None
        again = sc.run(lib, jobs, alpha, "cuda", fill, t if fill else 0.0)
        back = sc.run(lib, jobs[::-1], alpha, "cuda", fill, t if fill else 0.0)
        assert same((out, hole, raw), again[:3]) and not again[3].any(), case
        assert same((out, hole, raw), back[:3]) and not back[3].any(), case          # the same fill maps in the same order
    print(f"{kind}: {len(cases)} cases, worst err / bound {worst:.4f}; alpha > 0: {differ} of {values} values differ from the "
          f"emulation; reached in all: {sorted(union)}")
    assert {"batched_columns", "three_columns", "narrow_map", "width_is_window", "clipped_centre"} <= union
    assert {"centre_bad": {"centre_unplaced"}, "torn_x": {"direct_x", "split_pixel"}, "torn_y": {"direct_y", "split_pixel"},
            "margin": {"direct_x", "direct_y", "split_pixel"}, "back": {"negative_origin"}}[kind] <= union


def test_same_bits_on_every_run_and_under_every_job_order(lib):
    """The same call twice and the call with its jobs reversed: out, the hole byte and the raw sums are the same bits, `collapse`
    at 64x128 (every pixel of four jobs onto one target) included."""
    for kind, shape in (("collapse", (1, 64, 128)), ("noise", (2, 24, 48)), ("poles", (2, 17, 37))):
        jobs = sc.case_inputs(kind, shape, 0.25, 0.5, 3, 4)
        a = sc.run(lib, jobs, 0.5, "cuda")
        b = sc.run(lib, jobs, 0.5, "cuda")
        c = sc.run(lib, jobs[::-1], 0.5, "cuda")
        assert same(a[:3], b[:3]) and same(a[:3], c[:3]), kind
        assert not a[3].any() and not c[3].any()


def test_sums_are_zero_after_a_call_and_outputs_are_overwritten(lib):
    """sc.run fills out with NaN and hole with 255 beforehand: nothing of either is left, holes and masked sources included, and
    the sums are all-zero again, so a second call on the same buffers gives the first call's bits."""
    for shape in sr.SHAPES:
        B, H, W = shape
        jobs = sc.case_inputs("poles", shape, 0.5, 0.0, 4, 2)
        tj = sc.to_device(jobs, "cuda")
        acc = torch.zeros(B, 6, H, W, dtype=torch.int64, device="cuda")
        first = sc.run(lib, jobs, 0.0, "cuda", tjobs=tj, acc=acc)
        assert first[2].any() and not first[3].any() and not acc.any()
        assert int(first[1].max()) <= 1 and first[1].any() and not np.isnan(first[0]).any()
        again = sc.run(lib, jobs, 0.0, "cuda", tjobs=tj, acc=acc)
        assert same(first[:3], again[:3])


def test_unaligned_maps_take_the_element_form(lib, emu):
    """An output (and fill maps) 4 bytes past a 16-byte boundary at a width that is a multiple of 4: resolve's one-pixel form,
    the emulation's quad-form bits."""
    from prior_flow_amd.interp import FrameInterpolator
    B, H, W, C, t = 2, 24, 48, 3, 0.25
    jobs = sr.inputs("seam", B, H, W, C, 2, t, with_metric=False)
    (s0, f0, _, _, _, _), (s1, f1, _, _, _, _) = sc.to_device(jobs, "cuda")

    def shifted(x):
        buf = torch.zeros(x.numel() + 1, device="cuda")
        v = buf[1:].view(x.shape)
        v.copy_(x)
        return v

    fi = FrameInterpolator(B, C, H, W, "cuda")
    out = shifted(torch.full((B, C, H, W), float("nan")))
    assert out.data_ptr() % 16 == 4
    got = fi.frame(shifted(s0), shifted(s1), f0, f1, t, out=out)
    want = sc.run(emu, [dict(jobs[0], mask=None), dict(jobs[1], mask=None)], 0.0, fill=(jobs[0]["src"], jobs[1]["src"]), fill_t=t)
    assert np.array_equal(bits(got[0].cpu().numpy()), bits(want[0])) and np.array_equal(got[1].cpu().numpy(), want[1])
    assert not fi.acc.any()


def test_python_layer_on_the_device():
    from prior_flow_amd._lib import PfError
    from prior_flow_amd.interp import FrameInterpolator, splat
    B, C, H, W = 1, 3, 8, 16
    f = torch.rand(B, C, H, W, device="cuda") * 255
    z = torch.zeros(B, 2, H, W, device="cuda")
    fi = FrameInterpolator(B, C, H, W, "cuda")
    out, hole = fi.frame(f, f, z, z, 0.5)
    assert out.shape == f.shape and hole.dtype == torch.uint8 and not hole.any()
    for bad in (lambda: splat(f.cpu(), z.cpu()), lambda: splat(f, z.cpu()), lambda: splat(f, z[:, :1]),
                lambda: splat(f.double(), z), lambda: splat(f, z, mask=torch.zeros(B, H, W, device="cuda")),
                lambda: splat(f[:, :, :, ::2], z[:, :, :, ::2]), lambda: splat(f, z, metric=torch.zeros(B, 3, H, W, device="cuda")),
                lambda: fi.frame(f.cpu(), f, z, z, 0.5), lambda: fi.frame(f, f, z, z, 0.5, out=f),
                lambda: fi.frame(f, f, z, z.transpose(2, 3).contiguous().transpose(2, 3), 0.5),
                lambda: fi.frame(f, f, z, z, 1.0), lambda: fi.frame(f[:, :2], f[:, :2], z, z, 0.5),
                lambda: FrameInterpolator(B, C, H, W, "cpu"), lambda: FrameInterpolator(B, C, H, W, "cuda", vmax=0.5)):
        with pytest.raises(PfError):
            bad()
    assert not fi.acc.any()                              # a refused call has launched nothing


# ---- FrameInterpolator behind the bidirectional stream --------------------------------------------------------------------------
def test_interpolator_behind_the_stream_eager_and_captured():
    """A four-frame 128x256 sequence, iters = 2, occlusion "plane": from_bidirectional at t = 0.5 equals frame() on the returned
    tensors; a captured call replayed twice gives the eager call's bits; with zero flows and the same frame on both sides the
    result is the frame (to the integer quantum: 2^-33); splat(frame0, forward, 1.0) against frame1 is finite where it is neither
    a hole nor occluded -- its mean error is printed, not gated: the synthetic weights promise nothing about it."""
    from prior_flow_amd.interp import FrameInterpolator, splat
    from prior_flow_amd.modules import state_dict_shapes
    from prior_flow_amd.prior_raft import PriOr_RAFT
    from prior_flow_amd.video import BidirectionalFlow, FlowStream
    B, H, W = 1, 128, 256
    m = PriOr_RAFT(argparse.Namespace(mixed_precision=False, dropout=0.0, alternate_corr=False))
    m.load_state_dict(gc.det_state_dict(state_dict_shapes()), strict=True)
    m = m.cuda().eval()
    f0, _ = gc.synthetic_pair(B, H, W, seed=5)
    frames = [torch.roll(f0, shifts=(t, 3 * t), dims=(2, 3)).cuda().contiguous() for t in range(4)]
    stream = FlowStream(m, iters=2, bidirectional=True, occlusion="plane")
    fi, plain = FrameInterpolator(B, 3, H, W, "cuda"), FrameInterpolator(B, 3, H, W, "cuda")
    results, eager = [], []
    with torch.no_grad():
        for i, frame in enumerate(frames):
            r = stream(frame)
            if r is None:
                continue
            r = BidirectionalFlow(*[t.clone() for t in r])
            out, hole = fi.from_bidirectional(r, frames[i - 1], frame, 0.5)
            want = plain.frame(frames[i - 1], frame, r.forward, r.backward, 0.5, r.residual_forward, r.residual_backward)
            assert torch.equal(out, want[0]) and torch.equal(hole, want[1]) and bool(torch.isfinite(out).all())
            assert not fi.acc.any()
            results.append(r)
            eager.append((out.clone(), hole.clone()))
    assert len(results) == 3
    # the third call again, captured, replayed twice on copied-in inputs
    cap = FrameInterpolator(B, 3, H, W, "cuda")
    src = BidirectionalFlow(*[torch.zeros_like(t) for t in results[2]])
    a, b = torch.zeros_like(frames[2]), torch.zeros_like(frames[3])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        cap.from_bidirectional(src, a, b, 0.5, use_occlusion=False)            # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap.from_bidirectional(src, a, b, 0.5, use_occlusion=False)
    for s, t in zip(src, results[2]):
        s.copy_(t)
    a.copy_(frames[2])
    b.copy_(frames[3])
    for _ in range(2):
        cap.out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(cap.out, eager[2][0]) and torch.equal(cap.hole, eager[2][1]) and not cap.acc.any()
    # zero flows, the same frame on both sides: the frame itself
    z = torch.zeros(B, 2, H, W, device="cuda")
    out, hole = fi.frame(frames[1], frames[1], z, z, 0.5)
    assert not hole.any() and float((out - frames[1]).abs().max()) <= 2.0 ** -33
    # one frame carried along the forward flow
    r = results[0]
    out, hole = splat(frames[0], r.forward, 1.0)
    keep = (hole == 0) & (r.occ_backward == 0)
    err = float((out - frames[1]).abs().mean(1)[keep].mean())
    print(f"splat(frame0, forward) vs frame1: mean |error| {err:.3f} over {float(keep.float().mean()):.1%} of the pixels "
          f"({float((hole != 0).float().mean()):.1%} holes)")
    assert np.isfinite(err)
