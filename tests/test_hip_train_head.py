"""The head of the training tape -- both encoders (16 convolutions each through HipConv / HipConvS2 / HipSmallConv, the norms,
HipAddRelu), ContextSplit, SplitBatch, the two HipCorrPyramid nodes and the gradient sink's routes -- against a float64
reference pinned to the ReLU state of the run under test.  tests/train_head_ref.py says what is pinned and where the bounds come
from; test_train_head_reference.py proves on the CPU that they catch a transposed volume gradient, a lost row of a stride-2
backward, a normalisation backward without one of its terms.

The product's own path is driven: autograd.train_forward with train_loop.run_loop replaced by a stub that hands back what it was
given.  Graph replay is test_graphed_training_step_equals_the_eager_one's business."""
import argparse
import types

import pytest
import torch

import golden_cases as gc
import train_head_ref as th

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rig():
    """A real PriOr_RAFT in train() + freeze_bn() with det_state_dict weights and its flat optimizer (never stepped: the
    parameters' .grad are views of its gradient buffer, which is what the gradient sink writes into)."""
    from prior_flow_amd import train as tr
    from prior_flow_amd.modules import state_dict_shapes
    from prior_flow_amd.prior_raft import PriOr_RAFT
    m = PriOr_RAFT(argparse.Namespace(mixed_precision=False, dropout=0.0))
    m.load_state_dict(gc.det_state_dict(state_dict_shapes()), strict=True)
    m = m.cuda().train()
    m.freeze_bn()
    opt, _ = tr.fetch_optimizer(argparse.Namespace(lr=1e-4, wdecay=5e-5, epsilon=1e-8, num_steps=1000, clip=1.0), m)
    return m, opt


# ---------------------------------------------------------------------------------------------------------------------
# 1. the correlation node alone
# ---------------------------------------------------------------------------------------------------------------------
def _node_inputs(B, H, W, C=256, seed=5):
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: (torch.rand(*s, generator=gen, dtype=torch.float32) * 2 - 1).cuda()      # noqa: E731
    f1, f2 = r(B, C, H, W).requires_grad_(True), r(B, C, H, W).requires_grad_(True)
    seeds = [r(B * H * W, (H >> i) * (W >> i)) for i in range(4)]
    return f1, f2, seeds


def _node_check(what, got, want):
    fails = []
    for k in ("d_f1", "d_f2"):
        ref, tol_e, tol_a = want[k]
        assert got[k].shape == ref.shape and bool(torch.isfinite(got[k]).all()), k
        err = (got[k].double() - ref).abs()
        re, ra = float((err / tol_e).max()), float((err / tol_a).max())
        print(f"{what} {k}: worst |err| / per-element bound {re:.3f}, / aggregate bound {ra:.3f}; |ref| {float(ref.norm()):.3e}")
        if re > 1 or ra > 1:
            fails.append((k, re, ra))
    assert not fails, fails


@pytest.mark.parametrize("B,H,W", [(2, 16, 32), (1, 17, 27), (2, 17, 18)], ids=["B2_16x32", "B1_17x27_n459", "B2_17x18_n306"])
def test_corr_pyramid_node_backward(B, H, W):
    """ag.corr_pyramid on seeded leaf features, hand-made level gradients in the accumulator, backward through the token:
    d f1 and d f2 element by element against float64 under both bounds of train_head_ref.volume_grad_fp64 (K = n; the three
    additions of pf_pyramid_bwd and the scale are counted there).  n = 512: no K padding, two images; n = 459 (n % 4 == 3) and
    n = 306 (n % 4 == 2) take the F.pad route, the second with a live batch index."""
    from prior_flow_amd import autograd as ag
    f1, f2, seeds = _node_inputs(B, H, W)
    with th.clean_tape():
        levels, tok, acc = ag.corr_pyramid(f1, f2)
        for buf, s in zip(acc.buffers(levels), seeds):
            buf.copy_(s)
        tok.backward(torch.zeros_like(tok))
        torch.cuda.synchronize()
    want = th.volume_grad_fp64(f1.detach(), f2.detach(), seeds, B, H, W)
    _node_check(f"{B}x{H}x{W}", {"d_f1": f1.grad, "d_f2": f2.grad}, want)


def test_corr_pyramid_node_backward_at_n_90():
    """B = 2, 9x10: n = 90, n % 4 == 2, K padded to 92 -- below one K tile of the GEMM.  The forward (pf_corr_pyramid_bf16x3)
    refuses maps whose level 3 is smaller than 2x2, so ag.corr_pyramid cannot be called here; HipCorrPyramid.backward is, on a
    context that holds what the forward would have saved (the feature rows, the shape, the accumulator)."""
    from prior_flow_amd import autograd as ag
    B, H, W = 2, 9, 10
    f1, f2, seeds = _node_inputs(B, H, W)
    acc = ag.PyramidGrad()
    for buf, s in zip(acc.buffers(seeds), seeds):
        buf.copy_(s)
    ctx = types.SimpleNamespace(saved_tensors=(ag._rows(f1.detach()), ag._rows(f2.detach())), shape=(B, 256, H, W), acc=acc)
    with th.clean_tape():
        d1, d2, _ = ag.HipCorrPyramid.backward(ctx)
        torch.cuda.synchronize()
    want = th.volume_grad_fp64(f1.detach(), f2.detach(), seeds, B, H, W)
    _node_check("2x9x10", {"d_f1": d1, "d_f2": d2}, want)


def test_corr_pyramid_node_backward_with_an_empty_accumulator():
    """No lookup contributed (take() returns None): exact zeros of the features' shapes."""
    from prior_flow_amd import autograd as ag
    f1, f2, _ = _node_inputs(2, 16, 32)
    with th.clean_tape():
        levels, tok, acc = ag.corr_pyramid(f1, f2)
        assert acc.take() is None
        tok.backward(torch.zeros_like(tok))
        torch.cuda.synchronize()
    for f in (f1, f2):
        assert f.grad.shape == f.shape and f.grad.dtype == torch.float32 and not bool(f.grad.any())


# ---------------------------------------------------------------------------------------------------------------------
# 2. - 4. the assembly
# ---------------------------------------------------------------------------------------------------------------------
def _reference(h, case, weights, bn_train=False):
    ref, model = th.reference_and_model(case, weights, h.img_f, h.img_c, h.seeds, h.pins(), h.dev, bn_train)
    names = [k for k, _ in h.params()]
    assert len(names) == th.N_PARAMS and set(names) == set(ref[1])      # norm3 / downsample.1 once
    # the absolute term of `check` goes to the gradients that are exactly zero and to nothing else
    assert th.below_abs_term(ref[1]) == th.zero_gradient_names(names, bn_train)
    return ref, model


def _check(what, h, ref, model, grads=None):
    assert set(h.rec) | {"cnet.inp"} == set(th.relu_keys())
    f_fails, f_rep = th.check(h.forward(), ref[0], model[0])
    got = h.gradients() if grads is None else grads
    b_fails, b_rep = th.check(got, ref[1], model[1])
    print(f"{what}: forward worst err / bound: {th.worst(f_rep)}; backward: {th.worst(b_rep, 4)}; by group: {th.by_group(b_rep)}; "
          f"old metric {th.old_metric(got, ref[1]):.1e}")
    assert not f_fails, f_fails
    assert not b_fails, b_fails


@pytest.mark.parametrize("sink", [False, True], ids=["autograd", "sink"])
@pytest.mark.parametrize("case", [th.EVEN, th.RAGGED], ids=lambda c: c.name)
def test_head_is_the_vjp_at_its_relu_state(case, sink, rig, monkeypatch):
    """cnet frozen (freeze_bn, the default training configuration).  Sink off: every parameter gradient arrives through
    autograd's own accumulation; sink on: through GradSink as train.train_step does it (the step asserts that it started) --
    the stems and the frozen BatchNorms then add straight into .grad."""
    model, opt = rig
    with th.clean_tape():
        h = th.Harness(model, opt, case, monkeypatch)
        weights = th.weights_of(model.fnet, model.cnet)
        h.step(sink)
        ref, mdl = _reference(h, case, weights)
        _check(f"{case.name} sink={int(sink)}", h, ref, mdl)


def test_head_with_batch_statistics(rig, monkeypatch):
    """cnet left in train(): HipBatchNormTrain.  Gradients as above, and the running statistics every BatchNorm of cnet leaves.

    Bound of a statistic t: K_AGG * ||model_t - ref_t|| (the activations that reach the layer carry the rounding of the
    convolutions in front of it; the rounding model updates its statistics in fp32 from its own) + the fp32 roundings of the
    update itself, u = 2^-24 each, per element:
      running_mean = 0.9 rm + 0.1 mean:  8 u (|0.9 rm| + |0.1 mean|) -- rstd and -mean * rstd stored as fp32 (2), mean =
        -shift / scale (1), the constants 0.1 and 0.9 (2), two products (2), one addition (1);
      running_var = 0.9 rv + 0.1 var n / (n - 1):  12 u (|0.9 rv| + 0.1 (var + eps) n / (n - 1)) -- rstd (counted twice by the
        square: 2), the square (1), the reciprocal (1), - eps (1), the constants 0.1, n / (n - 1) and 0.9 (3), three products
        (3), one addition (1).
    num_batches_tracked is exact."""
    model, opt = rig
    case = th.EVEN
    bufs = {k: v.clone() for k, v in model.cnet.state_dict().items()}
    try:
        model.cnet.train()
        with th.clean_tape():
            h = th.Harness(model, opt, case, monkeypatch)
            weights = th.weights_of(model.fnet, model.cnet)
            h.step(True)
            ref, mdl = _reference(h, case, weights, bn_train=True)
            _check(f"{case.name} batch statistics", h, ref, mdl)
            got = {"cnet." + k: v.detach().clone() for k, v in model.cnet.state_dict().items() if ".norm3." not in k}
        u, fails, worst = 2.0 ** -24, [], (0.0, "")
        assert len(ref[3]) == 45
        for k, r in ref[3].items():
            if k.endswith("num_batches_tracked"):
                assert int(got[k]) == int(r) == int(weights[k]) + 1, k
                continue
            r = r.double()
            pre = k.rsplit(".", 1)[0]
            old = weights[k].double().to(r.device)
            new = (r - 0.9 * old).abs()                       # 0.1 mean resp. 0.1 var n / (n - 1)
            if k.endswith("running_mean"):
                upd = 8 * u * ((0.9 * old).abs() + new)
            else:
                upd = 12 * u * ((0.9 * old).abs() + new + 0.1 * 1e-5)
            bound = th.K_AGG * float((mdl[3][k].double() - r).norm()) + float(upd.norm())
            err = float((got[k].double() - r).norm())
            worst = max(worst, (err / bound, k))
            if not err <= bound:
                fails.append(f"{k}: |err| {err:.3e} > bound {bound:.3e} (|ref| {float(r.norm()):.3e})")
            assert float((r - old).abs().max()) > 0, pre
        print(f"running statistics: worst err / bound {worst[0]:.3f} ({worst[1]})")
        assert not fails, fails
    finally:
        model.cnet.load_state_dict(bufs)
        model.freeze_bn()


def test_head_accumulates_into_existing_gradients(rig, monkeypatch):
    """A second forward + backward without zeroing, sink on: every gradient is twice the reference within twice its bound
    (halving is exact, so the halved gradients are held to the bounds as they are).  The stems and the frozen BatchNorms add
    into .grad in place; everything else goes through the flush."""
    model, opt = rig
    case = th.EVEN
    with th.clean_tape():
        h = th.Harness(model, opt, case, monkeypatch)
        weights = th.weights_of(model.fnet, model.cnet)
        h.step(True)
        once = h.gradients()
        h.step(True, zero=False)
        twice = h.gradients()
        ref, mdl = _reference(h, case, weights)
        live = set(twice) - th.below_abs_term(ref[1])
        assert all(float((twice[k] - once[k]).abs().max()) > 0 for k in live)
        _check(f"{case.name} two steps, halved", h, ref, mdl, grads={k: v / 2 for k, v in twice.items()})
