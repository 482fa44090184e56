"""The training loop's ONE autograd node (prior_flow_amd/train_loop.py: LoopFn, ~35 launches per iteration of its hand-written
backward plus 32 deferred weight-gradient launches, on three streams by default) against a float64 reference pinned to the
forward state the node saved -- tests/train_loop_ref.py says what is pinned and where the bounds come from;
test_train_loop_reference.py proves on the CPU that they catch a wrong column offset, a missing accumulation, a stale buffer.

The node is driven directly (train_loop.run_loop on seeded leaves and hand-made pyramid triples, no encoders), so all its
outputs are compared: 6 leaf gradients, 8 pyramid-level gradients, every update-block weight and bias gradient."""
import argparse

import pytest
import torch

import golden_cases as gc
import train_loop_ref as tl

pytestmark = pytest.mark.gpu

_INPUTS = {}


def _inputs(case):
    if case.name not in _INPUTS:
        _INPUTS[case.name] = tl.make_inputs(case)
    return _INPUTS[case.name]


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


def _compare(h, case, inputs, what):
    """Reads the state the forward saved, evaluates the pinned float64 reference and the rounding model on the device and
    compares the forward (mean end-point error) and every output of the backward (train_loop_ref.check).  Returns (report line,
    mean EPE, failures, the predictions): the caller asserts."""
    torch.cuda.synchronize()
    got, preds, state = h.gradients(), [p.detach().clone() for p in h.preds], h.state()
    ref, model, ref_preds = tl.reference_and_model(case, inputs, state, h.dev)
    assert len(ref) == 6 + 8 + 2 * (19 + 15) and len(preds) == 2 * case.iters
    epe = max(tl.mean_epe(a, b) for a, b in zip(preds, ref_preds))
    fails, report = tl.check(got, ref, model)
    line = (f"{what}: forward mean EPE {epe:.2e}; worst err / bound: {tl.worst(report, 4)}; "
            f"old metric {tl.old_metric(got, ref):.1e}")
    return line, epe, fails, preds


def _assert_close(line, epe, fails):
    """The forward to 1e-3 px mean end-point error (the suite's figure against the oracle; the values are mostly pinned, so
    this is a sanity check of the harness), every gradient within its bound."""
    print(line)
    assert epe < 1e-3, epe
    assert not fails, fails


_REPLAYED = {}      # split -> [(report line, EPE, failures, predictions) of replay 1, of replay 2]; passing captures only


def _schedule(monkeypatch, split):
    monkeypatch.setenv("PRIORFLOW_TRAIN_SPLIT", split)
    monkeypatch.setenv("PRIORFLOW_GRAD_SINK", "1")      # Harness.step asserts that the sink really started


def _eager_predictions(split, rig, monkeypatch):
    _schedule(monkeypatch, split)
    with tl.clean_tape():
        h = tl.Harness(*rig, tl.EVEN)
        h.load(_inputs(tl.EVEN))
        h.step(True)
        torch.cuda.synchronize()
        return [p.detach().clone() for p in h.preds]


@pytest.mark.parametrize("sink", [False, True], ids=["autograd", "sink"])
@pytest.mark.parametrize("split", ["1", "0"], ids=["split1", "split0"])
@pytest.mark.parametrize("case", [tl.EVEN, tl.RAGGED], ids=lambda c: c.name)
def test_loop_backward_is_the_vjp_at_its_saved_state(case, split, sink, rig, monkeypatch):
    """Both schedules (PRIORFLOW_TRAIN_SPLIT: two chains on three streams / one chain) with the weight gradients handed to
    autograd on the calling stream and through the gradient sink as train.train_step does it (fetch_optimizer, _grad_sink,
    backward, flush: the deferred weight gradients run on the side stream -- the product's default)."""
    _schedule(monkeypatch, split)
    with tl.clean_tape():
        h = tl.Harness(*rig, case)
        h.load(_inputs(case))
        h.step(sink)
        line, epe, fails, _ = _compare(h, case, _inputs(case), f"{case.name} split={split} sink={int(sink)}")
    _assert_close(line, epe, fails)


def test_loop_backward_with_only_the_last_predictions_seeded(rig, monkeypatch):
    """All-zero seeds for every prediction but the last of each branch: the heads of the earlier iterations contribute
    nothing and the hidden-state chain alone carries the gradient back."""
    case = tl.EVEN_LAST
    _schedule(monkeypatch, "1")
    with tl.clean_tape():
        h = tl.Harness(*rig, case)
        h.load(_inputs(case))
        h.step(True)
        res = _compare(h, case, _inputs(case), case.name)
    _assert_close(*res[:3])


def _replayed(split, rig, monkeypatch):
    """One capture per schedule, shared by the two tests below while it passes: forward + backward + sink flush of a FRESH
    harness (leaves that no eager step on the default stream has touched, see Harness.forget), captured the way
    train.GraphedTrainStep does it -- an eager warm-up on a side stream (lazy initialisations, the loop's workspace, the sink
    learns its arena size), the arena reserved OUTSIDE the capture --, replayed on the first input set and, the static inputs
    refreshed, on the second; after each replay everything is compared with the reference of that replay's inputs."""
    if split in _REPLAYED:
        return _REPLAYED[split]
    from prior_flow_amd.autograd import SINK
    _schedule(monkeypatch, split)
    case = tl.EVEN
    sets = (_inputs(tl.EVEN), _inputs(tl.EVEN_B))
    with tl.clean_tape():
        h = tl.Harness(*rig, case)
        h.load(sets[0])
        cur = torch.cuda.current_stream()
        warm = torch.cuda.Stream()
        warm.wait_stream(cur)
        with torch.cuda.stream(warm):
            h.step(True)
        cur.wait_stream(warm)
        h.forget()                      # the capture must create its own AccumulateGrad nodes, on the capturing stream
        sink = SINK.for_device(h.dev.index)
        sink.reserve(h.dev)
        arena = sink.arena              # the graph holds its raw pointer: alive for as long as the graph is
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            h.step(True)
        out = []
        for n, inputs in enumerate(sets):
            h.load(inputs)
            graph.replay()
            out.append(_compare(h, case, inputs, f"{case.name} split={split} replay {n + 1}"))
        torch.cuda.synchronize()
        del graph, arena
    if all(epe < 1e-3 and not fails for _, epe, fails, _ in out):
        _REPLAYED[split] = out          # a failing replay is not kept: whoever asks next captures again
    return out


@pytest.mark.parametrize("split", ["1", "0"], ids=["split1", "split0"])
def test_loop_backward_under_graph_replay(split, rig, monkeypatch):
    """Replayed twice, the static inputs refreshed with a second seeded set before the second replay (a stale read cannot
    pass): after each replay the saved state is read back and every output is checked against the reference of THAT replay's
    inputs.  A missing edge between the three streams becomes a missing edge between parallel branches of the graph, where
    nothing else orders them."""
    for line, epe, fails, _ in _replayed(split, rig, monkeypatch):
        _assert_close(line, epe, fails)


def test_train_split_leaves_the_predictions_bitwise(rig, monkeypatch):
    """The counterpart of test_split_branch_chains_leave_the_flow_bitwise for the training loop: the 2 * iters predictions of
    PRIORFLOW_TRAIN_SPLIT=1 are bit for bit those of =0, eager and in the two graph replays (the second on refreshed inputs) --
    the forward has no atomics, and co_groups = 1 must not change what a launch computes.

    This is NOT asserted for the backward: pf_upsample_flow_bwd, the lookup and warp backwards and the weight gradients
    accumulate with float atomics, so two runs of the SAME mode differ in the last bits.  The backward's two schedules are
    instead each held to the float64 bounds (the tests above)."""
    case = tl.EVEN
    runs = {}
    for split in ("0", "1"):
        runs[split] = [_eager_predictions(split, rig, monkeypatch)] + [r[3] for r in _replayed(split, rig, monkeypatch)]
    for what, a, b in zip(("eager", "replay 1", "replay 2"), runs["0"], runs["1"]):
        assert len(a) == len(b) == 2 * case.iters
        for k, (x, y) in enumerate(zip(a, b)):
            assert bool(torch.isfinite(x).all()) and float(x.abs().max()) > 0
            assert torch.equal(x, y), (what, k, float((x - y).abs().max()))
    # the refreshed inputs were really used, and a replay on the first set reproduces the eager run
    assert not torch.equal(runs["1"][1][-1], runs["1"][2][-1])
    for x, y in zip(runs["1"][0], runs["1"][1]):
        assert torch.equal(x, y)
