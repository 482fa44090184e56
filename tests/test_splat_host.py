"""Forward softmax splatting without a GPU: the exact facts of the statement, the host emulation of
pf_splat_accumulate / pf_splat_resolve (tests/emu/pf_emu_splat.cpp over csrc/pf_splat.h, the file the device kernels compile) held
to the float64 restatement (tests/splat_ref.py) over the sweep, the seeded faults, the scale rule, the refusals of the built library
and the Python layer (prior_flow_amd.interp) on the emulation's handle."""
import ctypes

import numpy as np
import pytest
import torch

import splat_cases as sc
import splat_ref as sr


@pytest.fixture(scope="module")
def emu():
    return sc.emu()


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _job(src, flow, tau, beta, metric=None, mask=None):
    return dict(src=src, flow=flow, metric=metric, mask=mask, tau=float(np.float32(tau)), beta=float(np.float32(beta)))


# ---- facts of the statement, each exact ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sr.SHAPES)
def test_zero_flow_is_the_exact_blend(emu, shape):
    """Zero flow, byte-valued frames, t = 0.25: 0.75 I0 + 0.25 I1 bit for bit, no holes, through FrameInterpolator.frame."""
    from prior_flow_amd.interp import FrameInterpolator
    B, H, W = shape
    rng = np.random.default_rng(3)
    i0, i1 = (torch.from_numpy(rng.integers(0, 256, (B, 3, H, W)).astype(np.float32)) for _ in range(2))
    z = torch.zeros(B, 2, H, W)
    fi = FrameInterpolator(B, 3, H, W, "cpu", lib=emu)
    out, hole = fi.frame(i0, i1, z, z, 0.25)
    assert np.array_equal(bits(out.numpy()), bits((0.75 * i0 + 0.25 * i1).numpy()))
    assert not hole.any() and not fi.acc.any()


@pytest.mark.parametrize("shape", sr.SHAPES)
def test_integer_flow_is_a_roll(emu, shape):
    """`integer` (u = 3, v = -2), one job, tau = 1: the source rolled with wrap, bit for bit; the two rows v pushes out are gone and
    the two rows uncovered at the other edge are holes (0 without a fill)."""
    B, H, W = shape
    rng = np.random.default_rng(4)
    src = rng.uniform(0, 255, (B, 3, H, W)).astype(np.float32)
    flow = np.stack([sr.flow_family("integer", H, W, rng)] * B)
    out, hole, raw, after = sc.run(emu, [_job(src, flow, 1.0, 1.0)], 0.0)
    want = np.roll(src, (-2, 3), (2, 3))
    assert np.array_equal(bits(out[:, :, :H - 2]), bits(want[:, :, :H - 2]))
    assert not hole[:, :H - 2].any() and hole[:, H - 2:].all() and not out[:, :, H - 2:].any()
    assert not after.any()


@pytest.mark.parametrize("kind", ("pan", "seam", "noise", "collapse"))
def test_mass_is_conserved_exactly(emu, kind):
    """Away from the poles nothing is dropped: the integer D summed over all targets equals the sum of the contributions
    llrintf(w b_k 2^S_D), recomputed here from the same fp32 products; likewise cov."""
    B, H, W = 1, 24, 48
    rng = np.random.default_rng(5)
    flow = sr.flow_family(kind, H, W, rng)
    flow[1] = np.clip(flow[1], -3, 3)
    y, x = np.mgrid[0:H, 0:W]
    keep = (y >= 4) & (y < H - 5)
    mask = (~keep).astype(np.uint8)[None]
    src = rng.uniform(0, 255, (B, 1, H, W)).astype(np.float32)
    tau, beta = np.float32(0.5), np.float32(0.75)
    _, _, raw, _ = sc.run(emu, [_job(src, flow[None], tau, beta, mask=mask)], 0.0)
    SD, _ = sr.scales(1, H, W)
    qx = x.astype(np.float32) + tau * flow[0]
    qy = y.astype(np.float32) + tau * flow[1]
    fx, fy = qx - np.floor(qx), qy - np.floor(qy)
    total_d = total_c = 0
    for bx in (np.float32(1) - fx, fx):
        for by in (np.float32(1) - fy, fy):
            bk = (bx * by).astype(np.float32)[keep]
            bk = bk[bk > 0]
            total_d += int(np.rint((beta * bk).astype(np.float32).astype(np.float64) * 2.0 ** SD).astype(np.int64).sum())
            total_c += int(np.rint((beta * bk).astype(np.float32).astype(np.float64) * 2.0 ** SD).astype(np.int64).sum())
    assert int(raw[0, 1].sum()) == total_d and int(raw[0, 2].sum()) == total_c and total_d > 0


def test_the_order_of_the_adds_does_not_matter(emu):
    """The same bits under a reversed and two permuted orders of the (job, pixel) items and under a permuted order of the jobs:
    the raw sums, out and the hole byte.  `collapse` piles every pixel onto one target."""
    for kind, shape in (("noise", (2, 24, 48)), ("collapse", (1, 64, 128)), ("poles", (2, 17, 37))):
        jobs = sc.case_inputs(kind, shape, 0.25, 0.5, 3, 4)
        try:
            emu._dll.pf_emu_splat_order(0)
            base = sc.run(emu, jobs, 0.5)
            for seed in (1, 7, 12345):
                emu._dll.pf_emu_splat_order(seed)
                got = sc.run(emu, jobs, 0.5)
                assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(base[:3], got[:3])), (kind, seed)
        finally:
            emu._dll.pf_emu_splat_order(0)
        got = sc.run(emu, [jobs[2], jobs[0], jobs[3], jobs[1]], 0.5)
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(base[:3], got[:3])), kind


# ---- the emulation against float64 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sr.FAMILIES)
def test_emulation_matches_float64_over_the_sweep(emu, kind):
    worst = und = 0.0
    n = 0
    for case in sr.sweep():
        if case[0] != kind:
            continue
        figs = sc.check_case(emu, *case)[3]
        worst = max([worst] + [f["err_over_tol"] for f in figs])
        und = max([und] + [f["undecided"] for f in figs])
        n += 1
    print(f"{kind}: {n} cases, worst err / bound {worst:.4f}, most undecided {und:.4%}")
    assert n == (36 if kind == "expand" else 54) * 3


@pytest.mark.parametrize("kind", sr.DEVICE_FAMILIES)
def test_emulation_matches_float64_on_the_window_cases(emu, kind):
    """The host twin of the device's window cases (sc.DEVICE_PATHS; tests/test_hip_splat.py): the emulation has no window, so
    this says that the reference and its bounds hold on these flows before the device is held to them.  `centre_far` is shown to
    be beyond the reference: every pixel undecided, which is why the device is held to the emulation's bits there."""
    worst = und = 0.0
    n = 0
    for case in sc.DEVICE_PATHS:
        if case[0] != kind:
            continue
        out, hole, raw, figs = sc.check_case(emu, *case)
        worst = max([worst] + [f["err_over_tol"] for f in figs])
        und = max([und] + [f["undecided"] for f in figs])
        assert raw.any() and not hole.all()
        n += 1
    print(f"{kind}: {n} cases, worst err / bound {worst:.4f}, most undecided {und:.4%}")
    assert n == len(sr.DEVICE_SHAPES) * len(sr.DEVICE_SETTINGS)
    if kind == "centre_bad":
        _, B, H, W = (sr.CENTRE_FAR[0],) + sr.CENTRE_FAR[1]
        jobs = sc.case_inputs(*sr.CENTRE_FAR)
        ref = sr.reference(jobs, 0, 0.0)
        print(f"centre_far: {1 - ref['decided'].mean():.1%} of the pixels undecided")
        assert not ref["decided"].any()
        out, hole, raw, after = sc.run(emu, jobs, 0.0)
        assert raw.any() and not after.any() and np.isfinite(out).all()


# ---- seeded faults ---------------------------------------------------------------------------------------------------------------
# fault -> the case it is seeded at: (kind, shape, t, alpha, C, njobs)
FAULT_AT = {
    "pole_clamped": ("poles", (2, 24, 48), 0.5, 0.0, 3, 2),
    "no_wrap": ("seam", (2, 24, 48), 0.5, 0.0, 3, 2),
    "tau_u_only": ("pan", (2, 17, 37), 0.25, 0.0, 1, 1),
    "cov_without_beta": ("noise", (2, 24, 48), 0.25, 0.0, 3, 2),
    "hole_on_d": ("pan", (2, 24, 48), 0.5, 0.5, 3, 2),
    "metric_cm1": ("noise", (1, 64, 128), 0.5, 0.5, 4, 2),
}


@pytest.mark.parametrize("fault", sr.FAULTS)
def test_seeded_fault_is_caught(emu, fault):
    """Each deviation seeded into the restatement puts the (right) emulation outside the bounds of the same `check` that the sweep
    passes: a clamped pole row, a column that does not wrap, tau on u only, beta missing from cov (seeded where beta = 2^-11 keeps
    every coverage below cmin), the hole test on D, the metric read as one plane where it has two."""
    kind, shape, t, alpha, C, njobs = FAULT_AT[fault]
    jobs = sc.case_inputs(kind, shape, t, alpha, C, njobs)
    if fault == "cov_without_beta":
        for q in jobs:
            q["beta"] = 2.0 ** -11
    out, hole, _, _ = sc.run(emu, jobs, alpha)
    sr.check(out[0], hole[0], sr.reference(jobs, 0, alpha), None, f"{fault}: the statement")
    with pytest.raises(AssertionError):
        sr.check(out[0], hole[0], sr.reference(jobs, 0, alpha, fault=fault), None, f"{fault}: seeded")


def test_seeded_faults_of_the_two_launches_are_caught(emu):
    """Scales off by one bit between accumulate and resolve (resolve told vmax = 512 where accumulate had 255: S_N one bit
    lower) and a resolve that did not clear the sums (a second accumulate onto the first call's sums): both land outside the
    bounds."""
    shape = (2, 24, 48)
    jobs = sc.case_inputs("pan", shape, 0.5, 0.0, 3, 2)
    ref = sr.reference(jobs, 0, 0.0)
    out, hole, _, _ = sc.run(emu, jobs, 0.0)
    sr.check(out[0], hole[0], ref, None, "the statement")
    out, hole, _, _ = sc.run(emu, jobs, 0.0, resolve_vmax=512.0)
    with pytest.raises(AssertionError):
        sr.check(out[0], hole[0], ref, None, "scales off by one bit")
    other = sc.case_inputs("noise", shape, 0.5, 0.0, 3, 2)
    acc = torch.zeros(2, 5, 24, 48, dtype=torch.int64)
    emu.splat_accumulate(sc.to_device(other), acc, 0.0, sr.ZMAX, sr.VMAX)        # the sums a call would have left behind
    out, hole, _, _ = sc.run(emu, jobs, 0.0, acc=acc)
    with pytest.raises(AssertionError):
        sr.check(out[0], hole[0], ref, None, "sums not cleared")


# ---- the scale rule ----------------------------------------------------------------------------------------------------------------
def test_scale_rule_cannot_overflow(emu):
    """At every (njobs, H, W, vmax) of the sweep and at 4 x 2048 x 4096: njobs H W vmax 2^S_N < 2^62 (and the same for D), exact
    integers; the library's function gives the restatement's scales."""
    geos = [(nj, H, W, v) for nj in sr.NJOBS for _, H, W in sr.SHAPES for v in (1.0, 255.0, 256.0, 1000.0, 65536.0)]
    geos += [(4, 2048, 4096, 255.0), (4, 2048, 4096, 65536.0), (1, 1, 1, 1.0)]
    for nj, H, W, v in geos:
        got = (ctypes.c_int * 2)()
        emu._dll.pf_emu_splat_scales(nj, H, W, v, got)
        SD, SN = sr.scales(nj, H, W, v)
        assert (got[0], got[1]) == (SD, SN), (nj, H, W, v)
        assert nj * H * W * (1 << SD) <= 1 << 62 and SN >= 0
        assert nj * H * W * int(np.ceil(v)) * (1 << SN) <= 1 << 62
        assert nj * H * W * int(np.ceil(v)) * (1 << SN) + 4 * nj * H * W < 1 << 63        # the roundings included
    assert sr.scales(2, 512, 1024) == (42, 34)


# ---- refusals of the built library, before any launch ------------------------------------------------------------------------------
def test_built_library_refuses_bad_arguments():
    """Host pointers, nothing is launched: -1 = PF_ERR_BAD_ARG, -2 = PF_ERR_BAD_SHAPE."""
    import __graft_entry__ as ge
    from prior_flow_amd import _lib
    d = _lib.PfLib(ge.build_hip(), require_cuda=False)._dll
    Fl = ctypes.c_float
    buf = [ctypes.cast((ctypes.c_double * 64)(), ctypes.c_void_p) for _ in range(8)]
    acc, src, flow, metric, out, hole, f0, f1 = buf

    def job(**kw):
        q = _lib.SplatJob()
        q.src, q.flow, q.metric, q.mask, q.cm, q.tau, q.beta = src, flow, None, None, 0, 0.5, 0.5
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    def accum(jobs=None, njobs=1, acc_=acc, B=1, C=1, H=2, W=2, alpha=0.0, zmax=12.0, vmax=255.0):
        arr = (_lib.SplatJob * 4)(*(jobs or [job()]))
        return d.pf_splat_accumulate(arr, njobs, acc_, B, C, H, W, Fl(alpha), Fl(zmax), Fl(vmax), None)

    assert d.pf_splat_accumulate(None, 1, acc, 1, 1, 2, 2, Fl(0), Fl(12), Fl(255), None) == -1
    assert accum(acc_=None) == -1
    assert accum(njobs=0) == -1 and accum(njobs=5) == -1
    assert accum(C=0) == -1 and accum(C=5) == -1
    assert accum([job(src=None)]) == -1 and accum([job(flow=None)]) == -1
    assert accum([job(metric=metric, cm=0)]) == -1 and accum([job(metric=metric, cm=3)]) == -1
    assert accum([job(tau=float("inf"))]) == -1 and accum([job(tau=float("nan"))]) == -1
    assert accum([job(beta=0.0)]) == -1 and accum([job(beta=1.5)]) == -1 and accum([job(beta=float("nan"))]) == -1
    assert accum([job(), job(beta=0.0)], njobs=2) == -1            # the second job is checked too
    assert accum(alpha=-1.0) == -1 and accum(alpha=float("nan")) == -1 and accum(zmax=-1.0) == -1
    assert accum(vmax=0.5) == -1 and accum(vmax=1.0e6) == -1
    assert accum([job(src=acc)]) == -1
    assert accum(B=0) == -2 and accum(H=0) == -2 and accum(W=0) == -2 and accum(H=1 << 15, W=1 << 15) == -2

    def resolve(acc_=acc, out_=out, hole_=hole, a=None, b=None, t=0.5, cmin=2.0 ** -10, njobs=1, B=1, C=1, H=2, W=2, vmax=255.0):
        return d.pf_splat_resolve(acc_, out_, hole_, a, b, Fl(t), Fl(cmin), njobs, B, C, H, W, Fl(vmax), None)

    assert resolve(acc_=None) == -1 and resolve(out_=None) == -1 and resolve(hole_=None) == -1
    assert resolve(a=f0) == -1 and resolve(b=f1) == -1            # one fill map without the other
    assert resolve(a=out, b=f1) == -1 and resolve(a=f0, b=out) == -1      # out aliasing a source
    assert resolve(out_=acc) == -1
    assert resolve(a=f0, b=f1, t=1.5) == -1
    assert resolve(cmin=0.0) == -1 and resolve(njobs=0) == -1 and resolve(njobs=5) == -1 and resolve(C=5) == -1
    assert resolve(vmax=0.0) == -1
    assert resolve(B=0) == -2 and resolve(H=1 << 15, W=1 << 15) == -2
    assert d.pf_splat_scratch_bytes(2, 3, 4, 8) == 2 * 5 * 4 * 8 * 8
    assert d.pf_splat_scratch_bytes(2, 5, 4, 8) == -2 and d.pf_splat_scratch_bytes(0, 3, 4, 8) == -2


# ---- the Python layer on the emulation's handle ------------------------------------------------------------------------------------
def test_python_layer_maps_onto_the_entry_points(emu):
    """splat() is one job with beta = 1; FrameInterpolator.frame is the two jobs (frame0, flow01, t, 1 - t), (frame1, flow10,
    1 - t, t) with the blend fill; from_bidirectional passes the residuals and masks; refusals raise PfError."""
    from prior_flow_amd._lib import PfError
    from prior_flow_amd.interp import FrameInterpolator, splat
    from prior_flow_amd.video import BidirectionalFlow
    B, H, W, C, t = 2, 24, 48, 3, 0.25
    jobs = sr.inputs("noise", B, H, W, C, 2, t, with_metric=True, dirty=False)
    T = lambda a: torch.from_numpy(a)                        # noqa: E731
    f0, f1, g0, g1 = T(jobs[0]["src"]), T(jobs[1]["src"]), T(jobs[0]["flow"]), T(jobs[1]["flow"])
    res0 = T(np.concatenate([jobs[0]["metric"], jobs[0]["metric"]], 1))        # two planes, like a residual
    res1 = T(jobs[1]["metric"])
    occ0, occ1 = (T((np.random.default_rng(s).random((B, H, W)) < 0.1).astype(np.uint8)) for s in (1, 2))
    out, hole = splat(f0, g0, tau=0.5, lib=emu)
    want = sc.run(emu, [_job(jobs[0]["src"], jobs[0]["flow"], 0.5, 1.0)], 0.0)
    assert np.array_equal(bits(out.numpy()), bits(want[0])) and np.array_equal(hole.numpy(), want[1])
    fi = FrameInterpolator(B, C, H, W, "cpu", alpha=0.5, lib=emu)
    r = BidirectionalFlow(g0, g1, occ0, occ1, res0, res1)
    got = fi.from_bidirectional(r, f0, f1, t, use_occlusion=True)
    two = [_job(jobs[0]["src"], jobs[0]["flow"], t, 1 - t, res0.numpy(), occ0.numpy()),
           _job(jobs[1]["src"], jobs[1]["flow"], 1 - t, t, res1.numpy(), occ1.numpy())]
    want = sc.run(emu, two, 0.5, fill=(jobs[0]["src"], jobs[1]["src"]), fill_t=t)
    assert np.array_equal(bits(got[0].numpy()), bits(want[0])) and np.array_equal(got[1].numpy(), want[1]) and not fi.acc.any()
    for b in range(B):
        sr.check(want[0][b], want[1][b], sr.reference(two, b, 0.5), sr.fill_blend(jobs[0]["src"][b], jobs[1]["src"][b], t), "frame")
    none = FrameInterpolator(B, C, H, W, "cpu", alpha=0.5, fill="none", lib=emu).from_bidirectional(r, f0, f1, t, importance=None)
    assert not none[0][:, 0][none[1] != 0].any()
    fi.acc.fill_(7)
    fi.reset()
    assert not fi.acc.any()
    for bad in (lambda: splat(f0, g0),                                            # a CPU tensor and the product's library
                lambda: fi.frame(f0, f1, g0, g1, 1.0), lambda: fi.frame(f0, f1, g0, g1, 0.0),
                lambda: fi.frame(f0[:, :2], f1, g0, g1, t), lambda: fi.frame(f0.double(), f1, g0, g1, t),
                lambda: fi.frame(f0.transpose(2, 3).contiguous().transpose(2, 3), f1, g0, g1, t),
                lambda: fi.frame(f0, f1, g0, g1, t, out=f0), lambda: fi.frame(f0, f1, g0, g1, t, mask0=occ0.float()),
                lambda: fi.from_bidirectional(g0, f0, f1, t), lambda: fi.from_bidirectional(r, f0, f1, t, importance="x"),
                lambda: FrameInterpolator(B, 5, H, W, "cpu", lib=emu), lambda: FrameInterpolator(B, C, H, W, "cpu", fill="x", lib=emu),
                lambda: FrameInterpolator(B, C, H, W, "cpu")):
        with pytest.raises(PfError):
            bad()
