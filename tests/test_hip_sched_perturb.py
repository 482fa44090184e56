"""Cross-queue ordering of the launch schedules, tested by delaying one queue at a time (tests/sched_perturb.py has the method
and the argument; tests/test_sched_perturb_host.py proves the choke point and simulates the d >= T claim).

Per case: T (host wall time of the undelayed eager call) and d (one delay, by device events, >= 1.25 T) are measured and printed
on a `[sched]` line with the queues and their launch counts; then, per victim queue, a decoy call on another input, a host
synchronise, and the call with a delay in front of every launch of the victim -- the result is the reference's bit for bit.  A
premature reader finds the decoy's values: wrong, finite, in range.  Training steps run with lr = 0 and are split into parts of
ordinals, one case each.  No NaN / +-1e30 poison here, no mutants in captured calls.

References come from a fresh EAGER SINGLE-QUEUE model (use_streams=False, use_graph=False).  As in tests/test_hip_state.py no model
that owns a graph is dropped before the end of its test.  Run with ``-m gpu``; PRIORFLOW_SCHED_TABLE=<file> writes the T / d table
(profiles/r16_sched_perturb.json is such a file)."""
import pytest
import torch

import sched_perturb as sp
import test_hip_state as ths
from test_hip_state import MODES, RAGGED, SMALLEST, build, flat, frames, init_flow, make_stream, mismatch, pair

pytestmark = pytest.mark.gpu

SEED_X, SEED_Y = 101, 202


@pytest.fixture(scope="module")
def params():
    from prior_flow_amd.modules import state_dict_shapes
    import golden_cases as gc
    yield gc.det_state_dict(state_dict_shapes())
    sp.write_table()


@pytest.fixture(scope="module")
def queues():
    """The caller's stream and the model's three side streams: four torch streams that demonstrably overlap pairwise.  (Streams
    share a few hardware queues; between two streams on one hardware queue no missing edge can show.)"""
    got = sp.concurrent_streams(4)
    assert got is not None, "no four streams out of 16 overlap pairwise: the perturbation could not show a race between some queues"
    return got


def roles(queues):
    """The queues of a call by name; "capture" is torch.cuda.graph's stream once there is one, every other handle is "other"."""
    r = {nm: s.cuda_stream for nm, s in zip(("caller", "s1", "s2", "sb"), queues)}
    r["capture"] = lambda: getattr(torch.cuda.graph.default_capture_stream, "cuda_stream", None)
    r["default"] = 0
    return r


def on(stream):
    """The calling stream of a case, behind what the default stream has enqueued so far."""
    stream.wait_stream(torch.cuda.current_stream())
    return torch.cuda.stream(stream)


def _busy(big, n):
    """Device work on the current stream (n passes over 256 MB), enqueued only: the host runs ahead (tests/test_hip_augment.py)."""
    for _ in range(n):
        big.mul_(1.0)


# ---- (a) the harness has teeth ------------------------------------------------------------------------------------------------------
N_TOY = 1 << 22


class Toy:
    """Two queues, elementwise entry points only, ordinary allocations.  RAW: the side queue produces p = relu(a + b), the calling
    queue consumes q = (p > 0 ? g : 0).  WAR: the side queue reads p (r = relu(p + b)), the calling queue then overwrites p
    (coords = src + delta into p's storage).  `wait` puts the edge in or leaves it out."""

    def __init__(self, lib, side, kind, wait):
        self.lib, self.side, self.kind, self.wait = lib, side, kind, wait
        g = torch.Generator().manual_seed(7)
        shapes = [(N_TOY,)] * 3 + [(1, 2, 1024, N_TOY // 2048), (1, 1024, N_TOY // 2048, 2)]
        self.sets = [[torch.randn(sh, generator=g).cuda() for sh in shapes] for _ in range(2)]
        self.a, self.b, self.g, self.src, self.delta = (torch.empty(sh, device="cuda") for sh in shapes)
        self.p, self.q = torch.empty(N_TOY, device="cuda"), torch.empty(N_TOY, device="cuda")
        self.coords = torch.empty(shapes[3], device="cuda")

    def load(self, k):
        """Input set k (0: the call's, 1: the decoy's)."""
        for t, v in zip((self.a, self.b, self.g, self.src, self.delta), self.sets[k]):
            t.copy_(v)

    def fresh(self):
        """The call's inputs behind the decoy: p and q still hold the decoy's results, which a race reads early."""
        self.load(0)
        torch.cuda.synchronize()
        return self()

    def __call__(self):
        lib, main, side = self.lib, torch.cuda.current_stream(), self.side
        side.wait_stream(main)
        if self.kind == "raw":
            with torch.cuda.stream(side):
                lib.add_relu(self.a, self.b, self.p)
            if self.wait:
                main.wait_stream(side)
            lib.relu_mask(self.g, self.p, self.q)
            main.wait_stream(side)
            return self.q.clone()
        self.p.copy_(self.a)                # p's content for the reader; same queue as the overwrite below
        side.wait_stream(main)
        with torch.cuda.stream(side):
            lib.add_relu(self.p, self.b, self.q)
        if self.wait:
            main.wait_stream(side)
        lib.coords_add(self.coords, self.delta, src=self.src)     # overwrites ...
        self.p.copy_(self.coords.view(-1))                          # ... p while the reader may still be at it
        main.wait_stream(side)
        return self.q.clone()

    def run(self, k):
        self.load(k)
        torch.cuda.synchronize()
        return self()


@pytest.mark.parametrize("kind", ["raw", "war"])
def test_seeded_faults_in_a_two_queue_toy_are_reported(kind):
    """A producer/consumer pair on two queues whose wait is left out on purpose, read-after-write and write-after-read: run_perturbed
    must report it, and must report nothing for the same toy with the wait in place.  Torch streams share a few hardware queues
    and two streams on one hardware queue serialise, so fresh side streams are tried, 8 at the most, until the fault shows."""
    from prior_flow_amd import _lib
    lib = _lib.PfLib(_lib.LIB_PATH, require_cuda=True)
    shown = None
    for attempt in range(8):
        side = torch.cuda.Stream()
        good, bad = Toy(lib, side, kind, True), Toy(lib, side, kind, False)
        want = good.run(0)
        torch.cuda.synchronize()
        row = sp.calibrate(lambda: good(), f"toy {kind} (side stream {attempt})")
        ok = sp.run_perturbed(good.fresh, lambda: good.run(1), want, mismatch, f"toy {kind}, wait in place", row=row)
        assert not ok, "\n".join(ok)        # whatever the queues: the intact toy is never reported
        lines = sp.run_perturbed(bad.fresh, lambda: bad.run(1), want, mismatch, f"toy {kind}, wait left out")
        print("\n".join(lines) if lines else f"[sched] toy {kind}: side stream {attempt} shows nothing (a shared hardware queue)")
        if any("delayed" in line for line in lines):
            shown = lines
            break
    assert shown, f"toy {kind}: no side stream out of 8 showed the seeded fault"
    # the victim that exposes it is the producer's (raw) / the reader's (war) queue: the side queue
    assert any("victim queue" in line and "delayed" in line for line in shown)


# ---- (b) the inference forward ------------------------------------------------------------------------------------------------------
_REF = {}


def ref(params, mode, B, H, W, what, seed, iters):
    """The step's result on a fresh eager single-queue model (test_hip_state.step_ref with use_streams=False)."""
    key = (mode, B, H, W, what, seed, iters)
    if key not in _REF:
        m = build(params, mode, use_graph=False, use_streams=False)
        with torch.no_grad():
            out = m(*pair(B, H, W, seed), iters=iters, test_mode=what != "all", init_flow=init_flow(B, H, W) if what == "init" else None)
        _REF[key] = [t.clone() for t in flat(out)]
        torch.cuda.synchronize()
    return _REF[key]


def forward_case(params, queues, mode, what, iters, B, H, W, captured, name):
    """One forward configuration through calibrate + run_perturbed; returns the mismatch lines."""
    X, Y = pair(B, H, W, SEED_X), pair(B, H, W, SEED_Y)
    kw = dict(iters=iters, test_mode=what != "all", init_flow=init_flow(B, H, W) if what == "init" else None)
    want = ref(params, mode, B, H, W, what, SEED_X, iters)
    side = tuple(queues[1:])
    models = [build(params, mode, use_streams=True, use_graph=captured, _side_streams=side)]

    def run(im):
        with torch.no_grad():
            return models[-1](*im, **kw)

    def run_eager(im):
        return ths.eager(models[-1], lambda: run(im))

    with on(queues[0]):
        return _forward_case(params, queues, mode, captured, name, X, Y, want, models, run, run_eager)


def _forward_case(params, queues, mode, captured, name, X, Y, want, models, run, run_eager):
    run_eager(Y)
    row = sp.calibrate(lambda: run_eager(X), name)
    if not captured:
        return sp.run_perturbed(lambda: run(X), lambda: run(Y), want, mismatch, name, row=row, roles=roles(queues))
    # captured: a new model per run, so that the capture itself happens under Perturb (the delays become nodes of the victim's
    # branch); the decoy dirties its workspace eagerly.  Every model lives to the end of the test.
    lines = sp.run_perturbed(lambda: run(X), lambda: run_eager(Y), want, mismatch, name, row=row, roles=roles(queues),
                             fresh=lambda: models.append(build(params, mode, use_streams=True, use_graph=True, _side_streams=tuple(queues[1:]))))
    assert all(len(m._graphs) == 1 for m in models[1:])
    torch.cuda.synchronize()
    return lines


@pytest.mark.parametrize("captured", [False, True], ids=["eager", "captured"])
@pytest.mark.parametrize("mode", list(MODES))
def test_forward_under_one_delayed_queue(params, queues, mode, captured):
    """test_mode forward at iters = 2 (a deferred B join and the last iteration's rejoin), B = 1 at 128x256, every mode, side
    streams on: eager, and captured under the perturbation.  Reference: a fresh eager single-queue model."""
    name = f"forward {mode} {'captured' if captured else 'eager'} iters=2 B=1 128x256"
    lines = forward_case(params, queues, mode, "graph", 2, 1, *SMALLEST, captured, name)
    assert not lines, "\n".join(lines)


@pytest.mark.parametrize("case", ["all_iters3", "iters3", "init_flow", "no_split_ab", "B2_136x216"])
def test_forward_paths_under_one_delayed_queue(params, queues, case, monkeypatch):
    """bf16x3, eager, the further paths: test_mode=False at iters = 3 (the non-split iteration with mask_b: forks 2, 4 and 8),
    test_mode at iters = 3 (a middle iteration), init_flow, PRIORFLOW_SPLIT_AB=0, and B = 2 at 136x216.  Reference as above."""
    what, iters, B, (H, W) = {"all_iters3": ("all", 3, 1, SMALLEST), "iters3": ("graph", 3, 1, SMALLEST), "init_flow": ("init", 2, 1, SMALLEST),
                              "no_split_ab": ("graph", 2, 1, SMALLEST), "B2_136x216": ("graph", 2, 2, RAGGED)}[case]
    if case == "no_split_ab":
        monkeypatch.setenv("PRIORFLOW_SPLIT_AB", "0")
    lines = forward_case(params, queues, "bf16x3", what, iters, B, H, W, False, f"forward bf16x3 eager {case}")
    assert not lines, "\n".join(lines)


# ---- (c) video --------------------------------------------------------------------------------------------------------------------
_STREAM_REF = {}


def stream_ref(params, warm, bi):
    """test_hip_state.stream_ref on a SINGLE-QUEUE model: a fresh eager stream over frames(77, (2, -5))."""
    if (warm, bi) not in _STREAM_REF:
        s = make_stream(build(params, "bf16x3", use_streams=False, use_graph=False), warm, bi, use_graph=False)
        with torch.no_grad():
            _STREAM_REF[warm, bi] = [[t.clone() for t in flat(s(f))] for f in frames(77, (2, -5))]
        torch.cuda.synchronize()
    return _STREAM_REF[warm, bi]


@pytest.mark.parametrize("captured", [False, True], ids=["eager", "captured"])
@pytest.mark.parametrize("warm,bi", [(True, False), (False, False), (True, True)], ids=["forward_warm", "forward_cold", "bidirectional"])
def test_flow_stream_under_one_delayed_queue(params, queues, warm, bi, captured):
    """A FlowStream over four 128x256 frames (forward-only warm and cold; bidirectional with occlusion="sphere"), the whole
    sequence as one call without a host synchronise between the frames.  The decoy is a different sequence, then reset().
    Captured: a new stream on a new model per run; the decoy runs eagerly, so the call's first steps run eagerly AND are
    captured under the perturbation, and its later steps replay those graphs.  Reference: a fresh eager stream on a fresh single-queue
    model (stream_ref above)."""
    want = stream_ref(params, warm, bi)
    seq, other = frames(77, (2, -5)), frames(5, (1, 3))
    streams = []

    def fresh():
        streams.append(make_stream(build(params, "bf16x3", _side_streams=tuple(queues[1:])), warm, bi, use_graph=False))

    def play(fs, graph):
        s = streams[-1]
        s.reset()
        s.use_graph = graph
        with torch.no_grad():
            out = [s(f) for f in fs]
        s.use_graph = False
        return out

    fresh()
    name = f"FlowStream {'bidirectional' if bi else 'forward'} warm={warm} {'captured' if captured else 'eager'}"
    with on(queues[0]):
        play(other, False)
        row = sp.calibrate(lambda: play(seq, False), name)
        lines = sp.run_perturbed(lambda: play(seq, captured), lambda: play(other, False), want, mismatch, name, row=row,
                                 roles=roles(queues), fresh=fresh if captured else None)
        torch.cuda.synchronize()
    assert not lines, "\n".join(lines)


# ---- (d) training -----------------------------------------------------------------------------------------------------------------
TRAIN_PARTS = 4                 # a training step's launches are split into this many contiguous parts of ordinals, one case each
GRAD_TOL = 1e-5                 # of the gradient's norm: the bound tests/test_hip_train_step.py puts on the weight-gradient kernels'
#                                 fp32 atomics (1e-7 measured there), which make the flat gradient irreproducible bit for bit


@pytest.fixture(scope="module")
def train_rig(params, queues):
    """A PriOr_RAFT in train() + freeze_bn(), its three training side streams set to the overlapping ones, and a flat optimizer
    with lr = 0: the whole step runs, AdamW included, and leaves the parameters as they are bit for bit, so that every run of a
    case -- decoys too -- starts from the same weights."""
    import argparse
    from prior_flow_amd import train as tr
    m = build(params, "bf16x3").train()
    m.freeze_bn()
    m._train_side_stream, m._loop_side_stream, m._loop_b_stream = queues[1:]
    opt, sched = tr.fetch_optimizer(argparse.Namespace(lr=0.0, wdecay=5e-5, epsilon=1e-8, num_steps=10 ** 6, clip=1.0), m)
    crit = tr.uniform_loss(*SMALLEST)
    batches = []
    for seed in (SEED_X, SEED_Y):
        gen = torch.Generator().manual_seed(seed)
        gt = (torch.rand(1, 2, *SMALLEST, generator=gen) * 6 - 3).cuda()
        batches.append(pair(1, *SMALLEST, seed) + (gt, torch.ones(1, *SMALLEST).cuda()))
    return m, opt, sched, crit, batches, opt.flat.detach().clone()


def train_result(loss, metrics, opt):
    """[loss and the forward's metrics (float64, exact), the pre-clip gradient norm, the flat gradient buffer]."""
    keys = sorted(k for k in metrics if k != "grad_norm")
    return [torch.tensor([float(loss)] + [float(metrics[k]) for k in keys], dtype=torch.float64),
            torch.tensor([float(metrics["grad_norm"])], dtype=torch.float64), opt.grad.detach().clone()]


def train_mismatch(got, want, what):
    """Loss and metrics bit for bit; the gradient (and its norm) within GRAD_TOL of the reference's norm."""
    if not torch.equal(got[0], want[0]):
        return f"{what}: loss / metrics {got[0].tolist()} differ from the reference's {want[0].tolist()}: a cross-queue edge is missing"
    rel = float((got[2].double() - want[2].double()).norm() / want[2].double().norm())
    reln = abs(float(got[1]) - float(want[1])) / float(want[1])
    if not (rel <= GRAD_TOL and reln <= GRAD_TOL):
        return f"{what}: the flat gradient differs from the reference's by {rel:.3e} of its norm (norm: {reln:.3e}): a cross-queue edge is missing"
    return None


def _train_env(monkeypatch, config):
    monkeypatch.setenv("PRIORFLOW_GRAD_SINK", "1")
    monkeypatch.setenv("PRIORFLOW_TRAIN_SPLIT", "0" if config == "split0" else "1")
    monkeypatch.setenv("PRIORFLOW_TRAIN_LOOP", "0" if config == "tape" else "1")


_TRAIN_REF = {}


@pytest.mark.parametrize("part", range(TRAIN_PARTS))
@pytest.mark.parametrize("config", ["split1", "split0", "tape"])
def test_train_step_under_one_delayed_queue(train_rig, queues, config, part, monkeypatch):
    """train.train_step, eager, iters = 2, B = 1 at 128x256: the loop node with the gradient sink and PRIORFLOW_TRAIN_SPLIT=1
    (the default), =0, and the per-node tape (PRIORFLOW_TRAIN_LOOP=0).  The backward runs on the calling thread
    (set_multithreading_enabled(False)) so that its torch ops pass the dispatch mode too.  One case delays, per victim queue, the
    launches of one of TRAIN_PARTS parts of the step.  Reference: the undelayed run of the same configuration; for split1 the
    serial form split0, to which tests/test_hip_train_loop.py pins its predictions bitwise (loss and metrics; the gradient, which
    fp32 atomics make irreproducible bit for bit, within GRAD_TOL of its norm of split1's own undelayed run)."""
    from prior_flow_amd import train as tr
    m, opt, sched, crit, (X, Y), flat0 = train_rig

    def step(batch):
        with torch.autograd.set_multithreading_enabled(False):
            loss, metrics = tr.train_step(m, opt, sched, crit, *batch, iters=2, clip=1.0)
        return train_result(loss, metrics, opt)

    with on(queues[0]):
        for c in ("split0", config):
            if c not in _TRAIN_REF:
                _train_env(monkeypatch, c)
                step(Y)
                _TRAIN_REF[c] = step(X)
        _train_env(monkeypatch, config)
        want = [_TRAIN_REF["split0" if config == "split1" else config][0]] + _TRAIN_REF[config][1:]
        name = f"train_step {config} iters=2 B=1 128x256, part {part + 1}/{TRAIN_PARTS}"
        step(Y)
        row = sp.calibrate(lambda: step(X), name)
        names = dict(zip(("caller", "s1", "s2", "sb"), (q.cuda_stream for q in queues)))
        lines = sp.run_perturbed(lambda: step(X), lambda: step(Y), want, train_mismatch, name, row=row, roles=names,
                                 window=(part, TRAIN_PARTS))
        torch.cuda.synchronize()
    assert torch.equal(opt.flat, flat0), "lr = 0 did not leave the parameters as they were"
    assert not lines, "\n".join(lines)


@pytest.mark.parametrize("part", range(TRAIN_PARTS))
def test_graphed_train_step_under_one_delayed_queue(train_rig, queues, part, monkeypatch):
    """One GraphedTrainStep (a single graph), iters = 2: per run a new stepper whose one warm-up call is the decoy; its second call
    captures the step under the perturbation -- the delays become nodes of the victim's branch -- and replays it.  Reference: the
    undelayed capture and replay of a stepper of its own.  Every stepper lives to the end of the test."""
    from prior_flow_amd import train as tr
    m, opt, sched, crit, (X, Y), flat0 = train_rig
    _train_env(monkeypatch, "split1")
    steppers = []

    def fresh():
        steppers.append(tr.GraphedTrainStep(m, opt, sched, crit, iters=2, clip=1.0, warmup=1, split=False))

    def step(batch):
        with torch.autograd.set_multithreading_enabled(False):
            loss, metrics = steppers[-1](*batch)
        return train_result(loss, metrics, opt)

    def eager(batch):
        with torch.autograd.set_multithreading_enabled(False):
            tr.train_step(m, opt, sched, crit, *batch, iters=2, clip=1.0)

    with on(queues[0]):
        if "graphed" not in _TRAIN_REF:
            fresh()
            step(Y)
            _TRAIN_REF["graphed"] = step(X)
            _TRAIN_REF["graphed_keep"] = steppers[-1]
        want = _TRAIN_REF["graphed"]
        name = f"GraphedTrainStep iters=2 B=1 128x256, part {part + 1}/{TRAIN_PARTS}"
        eager(Y)
        row = sp.calibrate(lambda: eager(X), name)
        lines = sp.run_perturbed(lambda: step(X), lambda: step(Y), want, train_mismatch, name, row=row, roles=roles(queues),
                                 window=(part, TRAIN_PARTS), fresh=fresh)
        torch.cuda.synchronize()
    assert all(s.graphs is not None and len(s.graphs) == 1 for s in steppers)
    assert torch.equal(opt.flat, flat0), "lr = 0 did not leave the parameters as they were"
    assert not lines, "\n".join(lines)


# ---- (e) mutants of the real schedule -------------------------------------------------------------------------------------------------
# Waits whose removal the perturbation cannot show, by (function, ordinal of the wait within that function over the two calls),
# each with the path that implies it.  An unlisted survivor fails the test; so does a listed mutant that IS reported.  (B's lookup
# waiting for `start`, which engine.py's comment in iteration_split calls queue steering, is NOT here: in eager mode it is what
# orders sb behind the encoders, and its mutant is reported.)
_IMPLIED_B = ("implied: the last iteration's flow chain has waited for B's deferred tail (s1.wait_event(b_prev)) and the calling "
              "stream for the flow chain (main.wait_event(flow_done))")
_IMPLIED_S1 = "implied: s1's last launch precedes flow_done, which the calling stream has waited for (main.wait_event(flow_done))"
SURVIVORS = {
    ("_encode", 1): "the FIRST call, behind a host synchronise: `ev` orders s2's coords copies behind the caller's earlier work, "
                    "and there is none; the same wait of the second call (_encode#5) is reported",
    ("_await_b", 0): _IMPLIED_B, ("_await_b", 1): _IMPLIED_B,
    ("iteration_split", 13): _IMPLIED_S1, ("iteration_split", 27): _IMPLIED_S1,
}
MUTANT_PARTS = 4


@pytest.fixture(scope="module")
def mutant_rig(params, queues):
    """The call that is mutated: TWO forwards back to back (pair Y, then pair X) with no host synchronise between them, so that
    the edges which order a call behind its predecessor have something to order."""
    m = build(params, "bf16x3", use_streams=True, use_graph=False, _side_streams=tuple(queues[1:]))
    X, Y, Z = (pair(1, *SMALLEST, sd) for sd in (SEED_X, SEED_Y, ths.SEED_Z))

    def run(*ims):
        with torch.no_grad(), torch.cuda.stream(queues[0]):       # (no wait here: DropWait counts the call's own)
            return [m(*im, iters=2, test_mode=True) for im in ims]

    run(Z)
    row = sp.calibrate(lambda: run(Y, X), "mutants: two forwards bf16x3 eager iters=2 back to back")
    run(Z)
    torch.cuda.synchronize()
    with sp.DropWait() as dry, sp.Perturb() as log:
        run(Y, X)
        torch.cuda.synchronize()
    return run, (X, Y, Z), row, dry.waits, list(log.counts())


@pytest.mark.parametrize("part", range(MUTANT_PARTS))
def test_every_wait_of_the_forward_is_load_bearing_or_listed(params, mutant_rig, part):
    """One mutant per wait that two eager bf16x3 forwards (iters = 2) execute back to back: DropWait(k), with the queue that
    recorded the skipped event as the victim first and, if that shows nothing, every other queue in turn (the producer the wait
    orders may sit behind a further hop).  Both results are compared.  Every mutant must be reported, except those SURVIVORS
    lists with their reason.  Never under capture."""
    run, (X, Y, Z), row, waits, queues = mutant_rig
    want = ref(params, "bf16x3", 1, *SMALLEST, "graph", SEED_Y, 2) + ref(params, "bf16x3", 1, *SMALLEST, "graph", SEED_X, 2)
    delay = sp.shared_delay()
    delay.passes = row["passes"]
    assert len(waits) == 38 and all(r in queues for _, _, _, _, _, r in waits), waits
    table, unlisted, rotten = [], [], []
    for k, fn, j, line, waiter, recorder in waits[part::MUTANT_PARTS]:
        shown = None
        for victim in [recorder] + [q for q in queues if q != recorder]:
            run(Z)
            torch.cuda.synchronize()
            with sp.DropWait(k) as dw, sp.Perturb(victim=victim, delay=delay) as p:
                out = run(Y, X)
                torch.cuda.synchronize()
            assert dw.dropped == (k, fn, j, line, waiter, recorder) and len(dw.waits) == len(waits) and p.injected
            if mismatch(out, want, "mutant"):
                shown = victim
                break
        listed = SURVIVORS.get((fn, j))
        table.append(f"[sched] mutant {k:2d} {fn}#{j} (line {line}): queue {queues.index(waiter)} waits for queue {queues.index(recorder)}: "
                     + (f"REPORTED with queue {queues.index(shown)} delayed" if shown is not None else f"survives -- {listed or 'NOT LISTED'}"))
        if shown is None and listed is None:
            unlisted.append((fn, j, line))
        if shown is not None and listed is not None:
            rotten.append((fn, j, line))
    print("\n".join(table))
    out = run(Y, X)                          # the intact schedule again: the mutants left nothing behind
    torch.cuda.synchronize()
    assert not mismatch(out, want, "intact")
    assert not unlisted, f"waits whose removal nothing shows, and that SURVIVORS does not list: {unlisted}"
    assert not rotten, f"SURVIVORS lists mutants that are reported: {rotten}"


# ---- (f) the caller's side of the contract ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("caller", ["default_stream", "side_stream"])
@pytest.mark.parametrize("form", ["eager", "captured", "flow_stream"])
def test_callers_contract_without_host_syncs(params, form, caller):
    """No delays, and no host synchronise between the steps: behind a backlog on the calling stream the inputs themselves are
    produced by a queued copy_, the call runs, its result is consumed by a queued copy_, the input tensors are overwritten in
    place with another pair as soon as the call has returned, and the next call follows back to back -- on the default stream
    and with the caller on a stream of its own.  Everything is compared at the end, with the single-queue references."""
    big = torch.ones(64 << 20, device="cuda")
    side = torch.cuda.Stream()
    if form == "flow_stream":
        want = stream_ref(params, True, False)
        seq = frames(77, (2, -5))
        s = make_stream(build(params, "bf16x3"), True, False, use_graph=True)
        with torch.no_grad():
            for f in frames(5, (1, 3)):      # the decoy sequence; it also captures the graphs
                s(f)
        s.reset()
        steps = [(f,) for f in seq]
        call = lambda f: s(f)  # noqa: E731
    else:
        m = build(params, "bf16x3", use_streams=True, use_graph=form == "captured")
        seeds = [SEED_X, SEED_Y, SEED_X]
        want = [ref(params, "bf16x3", 1, *SMALLEST, "graph", sd, 2) for sd in seeds]
        steps = [pair(1, *SMALLEST, sd) for sd in seeds]
        with torch.no_grad():
            m(*pair(1, *SMALLEST, ths.SEED_Z), iters=2, test_mode=True)       # the decoy (captures the graph)
        call = lambda a, b: m(a, b, iters=2, test_mode=True)  # noqa: E731
    torch.cuda.synchronize()
    kept = [None if not w else torch.full_like(w[0], 7.0) for w in want]
    stream = side if caller == "side_stream" else torch.cuda.current_stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream), torch.no_grad():
        ins = [torch.zeros_like(t) for t in steps[0]]
        _busy(big, 40)                       # the calling stream stays behind the host from here on
        for n, step in enumerate(steps):
            for dst, src in zip(ins, step):
                dst.copy_(src)               # the inputs are produced behind the backlog -- and overwrite the previous call's
            out = call(*ins)
            if kept[n] is not None:
                kept[n].copy_(out)           # the result's consumer
            else:
                assert out is None
            del out
        for dst in ins:
            dst.fill_(255.0)                 # the caller's in-place use of its own tensors right behind the last call
    torch.cuda.synchronize()
    problems = [mismatch(k, w, f"{form} on the {caller}, call {n}") for n, (k, w) in enumerate(zip(kept, want)) if k is not None]
    problems = [p for p in problems if p]
    assert not problems, "\n".join(problems)
