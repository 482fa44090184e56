"""The self-supervised criterion on an MI355X: pf_selfsup_loss_batch on the device against the float64
restatement (tests/selfsup_ref.py) under the bounds derived there and against the host emulation of the same header within twice
those bounds (not bit for bit: the two expf differ); reproducibility under repeated calls and other grids; poisoned buffers; NULL
gradient entries; the criterion captured into a graph; train_step_selfsup end to end.  Run with ``-m gpu``."""
import argparse
import math

import numpy as np
import pytest
import torch

import golden_cases as gc
import selfsup_cases as sc
import selfsup_ref as sr

pytestmark = pytest.mark.gpu

CASES = [(H, W, B, n, var) for (H, W) in sc.SHAPES for B, n, var in ((1, 1, "plain"), (2, 3, "plain"), (3, 1, "far"))]


@pytest.fixture(scope="module")
def emu():
    return sc.emu()


@pytest.fixture(scope="module")
def lib():
    from prior_flow_amd._lib import load
    return load()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64) if a.dtype == np.float64 else a


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def tbits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool((a.contiguous().reshape(-1).view(torch.uint8) == b.contiguous().reshape(-1).view(torch.uint8)).all())


def inputs(H, W, B, n, var="plain", masked=None):
    i1, i2 = sc.images(B, H, W)
    mask = sc.mask_of(B, H, W) if (B == 2 if masked is None else masked) else None
    return sc.flows(B, n, H, W, variant=var), i1, i2, sc.weight(H, W), mask, sc.gamma_weights(n)


@pytest.mark.parametrize("H,W,B,n,var", CASES)
def test_device_matches_float64_and_the_emulation(lib, emu, H, W, B, n, var):
    """The cases of tests/test_selfsup_host.py on the device: losses, partial sums, the count and every gradient element within the
    float64 bounds, for three chunk counts; against the emulation every gradient element within twice its bound.  Worst error /
    bound 0.037 (33 x 70, B = 2); the bits are not the emulation's."""
    fl, i1, i2, w, mask, iw = inputs(H, W, B, n, var)
    ref = sr.criterion(fl, i1, i2, w, mask, iw)
    worst, equal = 0.0, True
    for nblk in (1, 3, 7):
        g, p = sc.call(lib, fl, i1, i2, w, mask, iw, nblk=nblk, device="cuda")
        worst = max(worst, sc.check(g, p, ref, f"device {var} {H}x{W} B={B} nblk={nblk}"))
        ge, pe = sc.call(emu, fl, i1, i2, w, mask, iw, nblk=nblk)
        for i in range(n):
            free = np.broadcast_to(ref[i]["near"][:, None], g[i].shape)
            assert (np.abs(g[i] - ge[i]) <= 2 * ref[i]["e_grads"])[~free].all(), (nblk, i)
            equal = equal and same(g[i], ge[i])
        te, td = pe.sum(axis=(1, 2)), p.sum(axis=(1, 2))
        for i in range(n):
            assert abs(td[i, 0] - te[i, 0]) <= 2 * ref[i]["e_photo"] and abs(td[i, 1] - te[i, 1]) <= 2 * ref[i]["e_smooth"]
            assert same(td[i, 3], te[i, 3])
    print(f"device {var} {H}x{W} B={B} n={n}: worst error / bound {worst:.3f}; gradient bits equal to the emulation's: {equal}")


def test_same_bits_under_repeats_and_grids(lib):
    """Two runs, and grids of 1, 3 and the default number of workgroups, give the same gradient and partial-sum bits: which pixels
    make a chunk and in which order a chunk is added is fixed by nblk."""
    for (H, W, B, n, nblk) in ((33, 70, 2, 3, 7), (5, 130, 3, 1, 2), (32, 64, 1, 3, 64)):
        fl, i1, i2, w, mask, iw = inputs(H, W, B, n, "far", masked=True)
        g0, p0 = sc.call(lib, fl, i1, i2, w, mask, iw, nblk=nblk, device="cuda")
        for blocks in (0, 1, 3, 0):
            g, p = sc.call(lib, fl, i1, i2, w, mask, iw, nblk=nblk, device="cuda", blocks=blocks)
            assert same(p, p0) and all(same(a, b) for a, b in zip(g, g0)), (H, W, blocks)


def test_poisoned_outputs_and_null_gradients(lib):
    """grads and partials full of NaN or +-1e30 before the call give the bits of zero-filled ones (every element is written, none
    is read); a NULL grads entry, and no grads at all, leave the partial sums and the other terms' gradients unchanged."""
    H, W, B, n, nblk = 33, 70, 2, 3, 5
    fl, i1, i2, w, mask, iw = inputs(H, W, B, n, "far", masked=True)

    def run(fill, pfill, drop=None, none=False):
        grads = None if none else [None if i == drop else torch.full((B, 2, H, W), fill, device="cuda") for i in range(n)]
        part = torch.full((n, B, nblk, 4), pfill, dtype=torch.float64, device="cuda")
        return sc.call(lib, fl, i1, i2, w, mask, iw, nblk=nblk, device="cuda", grads=grads, partials=part, want_grads=not none)

    g0, p0 = run(0.0, 0.0)
    for fill, pfill in ((float("nan"), float("nan")), (1e30, -1e30), (-1e30, float("inf"))):
        g, p = run(fill, pfill)
        assert same(p, p0) and all(same(a, b) for a, b in zip(g, g0)), fill
    g, p = run(0.0, 0.0, drop=1)
    assert same(p, p0) and g[1] is None and same(g[0], g0[0]) and same(g[2], g0[2])
    g, p = run(0.0, 0.0, none=True)
    assert g is None and same(p, p0)


def test_criterion_captured_lazy_equals_eager(lib):
    """SelfSupervisedLoss with lazy=True captured into ONE graph and replayed twice (the second time on other inputs copied into
    the static tensors) gives the eager call's bits: loss, metrics and every gradient."""
    from prior_flow_amd.selfsup import SelfSupervisedLoss
    H, W, B, n = 33, 70, 2, 3
    fl, i1, i2, w, mask, iw = inputs(H, W, B, n, masked=True)
    fl2 = sc.flows(B, n, H, W, seed=1)
    cu = lambda a: torch.from_numpy(np.array(a)).cuda()     # noqa: E731
    crit = SelfSupervisedLoss(H, W)
    static = [cu(f) for f in fl]
    t1, t2, tm = cu(i1), cu(i2), cu(mask)
    want = []
    for flows in (fl, fl2):
        loss, m = crit([cu(f) for f in flows], t1, t2, tm, extro_info="A-")
        want.append((loss.clone(), m, [g.clone() for g in crit.grads]))
    crit(static, t1, t2, tm, extro_info="A-", lazy=True)             # the state of this shape: allocated outside the capture
    torch.cuda.synchronize()
    own = [g.data_ptr() for g in crit.grads]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss, m = crit(static, t1, t2, tm, extro_info="A-", lazy=True)
    grads = crit.grads
    assert len(crit._state) == 1 and [g.data_ptr() for g in grads] == own      # the state's own buffers, none made in the capture
    for k, flows in enumerate((fl, fl2)):
        for s, f in zip(static, flows):
            s.copy_(cu(f))
        for g in grads:
            g.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        wl, wm, wg = want[k]
        assert tbits(loss, wl) and all(tbits(a, b) for a, b in zip(grads, wg))
        assert all(float(m[key]) == wm[key] for key in wm), (m, wm)


# ---- end to end -----------------------------------------------------------------------------------------------------------------
H2, W2, ITERS = 128, 256, 3
ARGS = argparse.Namespace(lr=1e-4, wdecay=5e-5, epsilon=1e-8, num_steps=1000, clip=1.0)


def _model():
    """tests/test_hip_train_step.py's seeded model."""
    from prior_flow_amd.modules import state_dict_shapes
    from prior_flow_amd.prior_raft import PriOr_RAFT
    m = PriOr_RAFT(argparse.Namespace(mixed_precision=False, dropout=0.0))
    m.load_state_dict(gc.det_state_dict(state_dict_shapes()), strict=True)
    m = m.cuda().train()
    m.freeze_bn()
    return m


def _frames():
    from prior_flow_amd import synthetic_pair
    return tuple(t.cuda() for t in synthetic_pair(1, H2, W2, seed=31))


def _by_hand(model, opt, crit, image1, image2):
    """The step's sequence up to the gradients, spelled out: both orders of the pair, forward, the two criteria with the masks of
    forward_backward_check on the halves of the final predictions, autograd.backward into the sink, flush."""
    from prior_flow_amd import _lib
    from prior_flow_amd import train as tr
    from prior_flow_amd.engine import rotation_x
    from prior_flow_amd.video import forward_backward_check
    lib = _lib.load()
    B = image1.shape[0]
    opt.zero_grad()
    first, second = torch.cat([image1, image2]).contiguous(), torch.cat([image2, image1]).contiguous()
    grid = lib.sample_grid(torch.empty(2, H2, W2, device="cuda"), rotation_x(-math.pi / 2))
    first_b, second_b = (lib.img_rotate(x, grid, torch.empty_like(x)) for x in (first, second))
    sink = tr._grad_sink(opt)
    preds_a, preds_b = model(first, second, iters=ITERS)
    masks = []
    for p in (preds_a, preds_b):
        f = p[-1].detach()
        occ_fw, occ_bw, _, _ = forward_backward_check(f[:B], f[B:], metric="sphere")
        masks.append(torch.cat([occ_fw, occ_bw]))
    loss_a, _ = crit(preds_a, first, second, masks[0], 0.8, extro_info="A-")
    seeds = list(crit.grads)
    loss_b, _ = crit(preds_b, first_b, second_b, masks[1], 0.8, extro_info="B-")
    seeds += list(crit.grads)
    torch.autograd.backward(list(preds_a) + list(preds_b), seeds)
    sink.flush()
    return opt.grad.detach().clone(), loss_a + loss_b, seeds, masks


def test_train_step_selfsup_end_to_end():
    """128 x 256, iters = 3, B = 1: the step sees two pairs.  train_step_selfsup leaves in optimizer.grad the gradient of the same
    sequence spelled out by hand on a second copy of the seeded model: the criterion's seeds and the masks bit for bit, the flat
    gradient bit for bit where the backward is (printed), and within 1e-5 of its norm in any case -- the weight-gradient kernels
    of the backward add with atomics, whose run-to-run noise tests/test_hip_train_step.py measures at 1e-7 (measured here: 1.1e-6,
    bits not equal).  Every parameter
    gradient is finite, the total norm positive, no torch kernel in the tape, the parameters change and the next inference
    forward sees them."""
    from prior_flow_amd import autograd as ag
    from prior_flow_amd import selfsup as ss
    from prior_flow_amd import train as tr
    i1, i2 = _frames()
    model = _model()
    opt, sched = tr.fetch_optimizer(ARGS, model)
    crit = ss.SelfSupervisedLoss(H2, W2)
    with torch.no_grad():
        model.eval()
        flow_before = model(i1, i2, iters=ITERS, test_mode=True).clone()
        model.train()
        model.freeze_bn()
    before = opt.flat.detach().clone()
    ag.STATS["hip"] = ag.STATS["torch"] = 0
    loss, m = ss.train_step_selfsup(model, opt, sched, crit, i1, i2, iters=ITERS, clip=ARGS.clip)
    assert ag.STATS["hip"] > 0 and ag.STATS["torch"] == 0, ag.STATS
    got = opt.grad.detach().clone()
    assert math.isfinite(float(loss)) and torch.isfinite(got).all() and m["grad_norm"] > 0
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
    assert abs(float(got.double().norm()) - m["grad_norm"]) <= 1e-5 * m["grad_norm"]
    for k in ("A-photo", "A-smooth", "A-used", "A-left_out", "B-photo", "B-smooth", "B-used", "B-left_out"):
        assert math.isfinite(m[k]), k
    assert 0 < m["A-used"] <= 1 + 1e-6 and m["A-left_out"] == 0
    assert not torch.equal(opt.flat, before)
    with torch.no_grad():
        model.eval()
        flow_after = model(i1, i2, iters=ITERS, test_mode=True)
    assert torch.isfinite(flow_after).all() and not torch.equal(flow_after, flow_before)

    model2 = _model()
    opt2, _ = tr.fetch_optimizer(ARGS, model2)
    crit2 = ss.SelfSupervisedLoss(H2, W2)
    want, loss2, seeds, masks = _by_hand(model2, opt2, crit2, i1, i2)
    # the same forward, masks and seeds, replayed through the step's own pieces on a third copy: bit for bit
    model3 = _model()
    opt3, _ = tr.fetch_optimizer(ARGS, model3)
    first, second = torch.cat([i1, i2]), torch.cat([i2, i1])
    sink = tr._grad_sink(opt3)
    try:
        pa, pb = model3(first, second, iters=ITERS)
        ma, mb = ss.occlusion_masks(pa[-1]), ss.occlusion_masks(pb[-1])
        assert tbits(ma, masks[0]) and tbits(mb, masks[1])
        crit(pa, first, second, ma, 0.8, extro_info="A-")
        sa = list(crit.grads)
        crit(pb, ss.to_view_b(first), ss.to_view_b(second), mb, 0.8, extro_info="B-")
        assert all(tbits(a, b) for a, b in zip(sa + list(crit.grads), seeds))
    finally:
        sink.abort()
    rel = float((got - want).norm() / want.norm())
    print(f"train_step_selfsup against the sequence by hand: gradient bits equal {tbits(got, want)}, relative difference {rel:.2e}, "
          f"loss {float(loss):.6f} / {float(loss2):.6f}, norm {m['grad_norm']:.4f}, masked A {float(masks[0].float().mean()):.3f} "
          f"B {float(masks[1].float().mean()):.3f}")
    assert tbits(loss, loss2)
    assert rel <= 1e-5


def test_occlusion_none_and_a_failing_criterion():
    """occlusion="none" hands both criteria masks of zeros; an unknown mode is refused before anything runs; an exception raised
    inside the criterion leaves the gradient sink inactive with nothing queued, the gradients as zero_grad left them and the
    parameters untouched, and the next regular step runs."""
    from prior_flow_amd import selfsup as ss
    from prior_flow_amd import train as tr
    from prior_flow_amd._lib import PfError
    from prior_flow_amd.autograd import SINK
    i1, i2 = _frames()
    model = _model()
    opt, sched = tr.fetch_optimizer(ARGS, model)
    seen = []

    class Recording(ss.SelfSupervisedLoss):
        def __call__(self, preds, image1, image2, mask=None, *a, **k):
            seen.append(mask)
            return super().__call__(preds, image1, image2, mask, *a, **k)

    crit = Recording(H2, W2)
    with pytest.raises(PfError):
        ss.train_step_selfsup(model, opt, sched, crit, i1, i2, iters=2, occlusion="both")
    assert not seen
    _, m = ss.train_step_selfsup(model, opt, sched, crit, i1, i2, iters=2, occlusion="none")
    assert len(seen) == 2 and all(k.dtype == torch.uint8 and tuple(k.shape) == (2, H2, W2) and not k.any() for k in seen)
    assert m["A-used"] == pytest.approx(1.0, abs=1e-6) and m["grad_norm"] > 0

    class Boom(RuntimeError):
        pass

    def failing(*a, **k):
        raise Boom("criterion failed")

    flat = opt.flat.detach().clone()
    steps = opt.step_count
    with pytest.raises(Boom):
        ss.train_step_selfsup(model, opt, sched, failing, i1, i2, iters=2)
    assert not SINK.active and not SINK.jobs and not SINK.keep
    assert not opt.grad.any() and torch.equal(opt.flat, flat) and opt.step_count == steps
    _, m = ss.train_step_selfsup(model, opt, sched, crit, i1, i2, iters=2)
    assert math.isfinite(m["grad_norm"]) and m["grad_norm"] > 0 and not SINK.active and seen[-1].dtype == torch.uint8


def test_five_steps_on_one_pair_are_reported():
    """Five AdamW steps from the seeded weights on one pair, with the forward-backward masks and without: the photometric loss of the
    batch before and after is printed (DESIGN.md section 21 records it) and not asserted -- nobody knows yet what five steps from
    seeded weights do to it; the steps must run and stay finite.  `photo` is a sum over the pixels used, so under "fb" it moves with
    the masks (`used`) as well as with the residual; under "none" every pixel counts at every step."""
    from prior_flow_amd import selfsup as ss
    from prior_flow_amd import train as tr
    i1, i2 = _frames()
    keys = ("A-photo", "B-photo", "A-used", "B-used", "A-smooth", "B-smooth")
    for occlusion in ("fb", "none"):
        model = _model()
        opt, sched = tr.fetch_optimizer(ARGS, model)
        crit = ss.SelfSupervisedLoss(H2, W2)
        hist = []
        for _ in range(6):                      # the sixth call's metrics are the state after five steps
            loss, m = ss.train_step_selfsup(model, opt, sched, crit, i1, i2, iters=ITERS, occlusion=occlusion)
            assert math.isfinite(float(loss)) and math.isfinite(m["grad_norm"])
            hist.append([round(float(loss), 6)] + [round(m[k], 6) for k in keys])
        print(f"five steps, occlusion {occlusion} (loss, {', '.join(keys)}): before {hist[0]} after {hist[5]}")
