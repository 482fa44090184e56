"""The forward owes nothing to what an earlier call left in the resident buffers, and no call damages what must survive it.

Every device buffer of the product is allocated once with torch.zeros and reused.  tests/state_audit.py classifies every cell of
every such buffer; here the cells a call may not rely on (SCRATCH) are filled with NaNs, then with +-1e30, in front of each kind of
call -- graph capture, graph replay, eager test_mode, test_mode=False, init_flow, the training forward, video streams, the
training step -- and the call has to return, bit for bit, what a model that was never poisoned returns; afterwards the cells
that must survive (CONST, ZERO) are checked.

Every reference comes from a fresh EAGER model (use_graph=False), the captured path included: graph and eager are held to the
same bits.  The form in which each graph call is compared with a fresh model that CAPTURES its own graph is left out: building
such reference models and dropping them while their last replay was still running ended a run of this file with a segmentation
fault inside CUDAGraph.replay() of the next model, and the cause is not known.  No test here drops a
model that owns a graph except at its own end, behind the assertions' read-backs.

A mismatch is a product bug -- a kernel that reads a cell before anything wrote it, or writes one column too far.  To find the
launch, bisect the POISONED SET: ``state_audit.poison(audit, pattern, only=lambda name: ...)`` with half the names, then one
buffer, then one region, and read the kernels that consume it.  Run with ``-m gpu``."""
import argparse

import pytest
import torch

import golden_cases as gc
import state_audit as sa

pytestmark = pytest.mark.gpu

MODES = {"bf16x3": {}, "f16": dict(mixed_precision=True), "alt_corr": dict(alternate_corr=True),
         "f16_alt_corr": dict(mixed_precision=True, alternate_corr=True)}
SEED_X, SEED_Y, SEED_Z = 101, 202, 303
RAGGED = (136, 216)         # 17 x 27 at 1/8: partial conv tiles, a partial lookup tile, W8 % 4 == 3
SMALLEST = (128, 256)       # 16 x 32: the smallest shape a Workspace accepts


@pytest.fixture(scope="module")
def params():
    from prior_flow_amd.modules import state_dict_shapes
    return gc.det_state_dict(state_dict_shapes())


def build(params, mode, **attrs):
    from prior_flow_amd.prior_raft import PriOr_RAFT
    kw = MODES[mode]
    m = PriOr_RAFT(argparse.Namespace(mixed_precision=kw.get("mixed_precision", False), dropout=0.0,
                                      alternate_corr=kw.get("alternate_corr", False)))
    m.load_state_dict(params, strict=True)
    m = m.cuda().eval()
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


_PAIRS = {}


def pair(B, H, W, seed):
    key = (B, H, W, seed)
    if key not in _PAIRS:
        i1, i2 = gc.synthetic_pair(B, H, W, seed=seed)
        _PAIRS[key] = (i1.cuda(), i2.cuda())
    return _PAIRS[key]


def init_flow(B, H, W):
    """A smooth 1/8-resolution flow of up to 2.5 px: the lookups of the first iteration cross the seam."""
    ys, xs = torch.meshgrid(torch.arange(H // 8, dtype=torch.float32), torch.arange(W // 8, dtype=torch.float32), indexing="ij")
    f = torch.stack([2.5 * torch.sin(xs / 3.0 + ys / 5.0), 1.5 * torch.cos(ys / 2.0 - xs / 7.0)])
    return f[None].repeat(B, 1, 1, 1).contiguous().cuda()


def flat(out):
    """A call's result as a list of tensors: a flow, (preds_A, preds_B), a BidirectionalFlow, None."""
    if out is None:
        return []
    if isinstance(out, torch.Tensor):
        return [out.detach()]
    return [t for o in out for t in flat(o)]


def mismatch(got, want, what):
    """None when the two results are equal bit for bit, else the line that says where they are not."""
    got, want = flat(got), flat(want)
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k)
        if not torch.equal(g, w):
            bad = g != w
            return (f"{what}: output {k} differs from a never-poisoned model's in {int(bad.sum())} of {g.numel()} elements "
                    f"({int((~torch.isfinite(g.float())).sum())} not finite; first at {tuple(int(v) for v in bad.nonzero()[0])}): "
                    "the call read resident state that it had not written -- bisect the poisoned set (module docstring)")
    return None


def conclude(problems, audit, snap):
    """The mismatches of a test and, whether there were any or not, the damage to CONST / ZERO regions: one assertion, so that a
    stray write is reported by the name of the buffer even where it also changed a result."""
    problems = [p for p in problems if p] + sa.failures(audit, snap)
    assert not problems, "\n".join(problems)


def assert_poisoned(a, names):
    """The poison really sits in the SCRATCH cells of the named buffers (a renamed or skipped attribute must not pass in silence)."""
    for name in names:
        e = a.entry(name)
        v = e.owner[e.scratch_mask()]
        assert v.numel() > 0, name
        if v.dtype.is_floating_point:
            v = v.double()
            assert bool((~torch.isfinite(v) | (v.abs() > 5e4)).all()), name
        else:
            assert bool(((v == -1) | (v == 0x7fffffff)).all()), name


def model_audit(m, *more, clean=True):
    """Every workspace of the model and every buffer set of both encoder plans (+ further containers)."""
    cs = [(f"ws{list(k[:3])}", ws) for k, ws in m._ws.items()]
    if m._enc_plans is not None:
        cs += [("cnet", m._enc_plans[0]), ("fnet", m._enc_plans[1])]
    return sa.audit(*cs, *more, clean=clean)


def eager(m, fn):
    keep, m.use_graph = m.use_graph, False
    try:
        return fn()
    finally:
        m.use_graph = keep


# ---- (a) + (b) poisoned workspace, call history ---------------------------------------------------------------------------------
_STEP_REF = {}


def step_ref(params, mode, B, H, W, what, seed, iters):
    """The step's result on a fresh EAGER model that is given nothing but that step's arguments."""
    key = (mode, B, H, W, what, seed, iters)
    if key not in _STEP_REF:
        m = build(params, mode, use_graph=False)
        im = pair(B, H, W, seed)
        if what == "train":
            m.train()
            m.freeze_bn()
            out = m(*im, iters=iters)
        else:
            with torch.no_grad():
                out = m(*im, iters=iters, test_mode=what != "all", init_flow=init_flow(B, H, W) if what == "init" else None)
        _STEP_REF[key] = [t.clone() for t in flat(out)]
    return _STEP_REF[key]


@pytest.mark.parametrize("poison", [None] + list(sa.PATTERNS), ids=["unpoisoned", "nan", "big"])
@pytest.mark.parametrize("B,H,W", [(1,) + RAGGED, (2,) + SMALLEST], ids=["B1_136x216", "B2_128x256"])
@pytest.mark.parametrize("use_streams", [True, False], ids=["streams", "one_stream"])
@pytest.mark.parametrize("mode", list(MODES))
def test_call_history_leaves_no_trace(params, mode, use_streams, B, H, W, poison):
    """One model through: graph capture (X), eager test_mode=False (Y: every B-branch and mask buffer), replay into the dirtied
    workspace (Y), init_flow (Z), a new capture on the dirty workspace (iters=2, X), a training step where the mode has one,
    replay (Z), replay (X) -- each result is a fresh eager model's for that step's arguments alone, the last equals the first.
    With a pattern, every SCRATCH cell of the workspace and of the encoders' buffer sets is poisoned in front of EVERY step.
    The workspace is built, and its CONST regions recorded, before the first launch."""
    m = build(params, mode, use_streams=use_streams)
    X, Y, Z = (pair(B, H, W, s) for s in (SEED_X, SEED_Y, SEED_Z))
    tag = f"{mode} B={B} {H}x{W} use_streams={use_streams} poison={poison}"
    problems = []
    with torch.no_grad(), torch.cuda.device(X[0].device):
        m._workspace(B, H, W, X[0].device)
    snap = sa.snapshot(model_audit(m))
    assert len(snap) == 6

    def dirty():
        if poison is not None:
            a = model_audit(m)
            assert sa.poison(a, poison) > 0
            assert_poisoned(a, [f"ws[{B}, {H}, {W}].{n}" for n in ("net0_ab", "x_ab_s", "cat_a_s", "mask_a", "pre[('b', '2')]", "c1a")])

    def step(n, what, seed, iters):
        dirty()
        im = pair(B, H, W, seed)
        with torch.no_grad():
            out = m(*im, iters=iters, test_mode=what != "all", init_flow=init_flow(B, H, W) if what == "init" else None)
        problems.append(mismatch(out, step_ref(params, mode, B, H, W, what, seed, iters), f"{tag}, step {n} ({what}, iters={iters})"))
        return flat(out)

    first = [t.clone() for t in step(1, "graph", SEED_X, 3)]
    step(2, "all", SEED_Y, 2)
    step(3, "graph", SEED_Y, 3)
    step(4, "init", SEED_Z, 1)
    step(5, "graph", SEED_X, 2)
    if "alternate_corr" not in MODES[mode]:             # (the training forward refuses alternate_corr)
        dirty()
        m.train()
        m.freeze_bn()
        pa, pb = m(*Y, iters=2)
        problems.append(mismatch((pa, pb), step_ref(params, mode, B, H, W, "train", SEED_Y, 2), f"{tag}, step 6 (training forward)"))
        (pa[-1].abs().sum() + pb[-1].abs().sum()).backward()
        m.eval()
        m.zero_grad(set_to_none=True)
        step(6, "graph", SEED_Z, 3)
    last = step(7, "graph", SEED_X, 3)
    problems.append(mismatch(last, first, f"{tag}, step 7 against step 1"))
    assert set(k[3] for k in m._graphs) == {2, 3}
    loop = [("loop", m._loop_bufs)] if getattr(m, "_loop_bufs", None) is not None else []
    conclude(problems, model_audit(m, *loop), snap)


# ---- (c) streams -----------------------------------------------------------------------------------------------------------------
def frames(seed, drift, T=4):
    f0, _ = gc.synthetic_pair(1, *SMALLEST, seed=seed)
    return [torch.roll(f0, shifts=(drift[0] * t, drift[1] * t), dims=(2, 3)).cuda() for t in range(T)]


def make_stream(m, warm, bi, **kw):
    from prior_flow_amd.video import FlowStream
    return FlowStream(m, iters=2, warm_start=warm, bidirectional=bi, occlusion="sphere" if bi else None, **kw)


_STREAM_REF = {}


def stream_ref(params, warm, bi):
    key = (warm, bi)
    if key not in _STREAM_REF:
        s = make_stream(build(params, "bf16x3"), warm, bi, use_graph=False)       # a fresh stream on a fresh model, eager
        with torch.no_grad():
            _STREAM_REF[key] = [[t.clone() for t in flat(s(f))] for f in frames(77, (2, -5))]
    return _STREAM_REF[key]


@pytest.mark.parametrize("pattern", sa.PATTERNS)
@pytest.mark.parametrize("warm", [True, False], ids=["warm", "cold"])
@pytest.mark.parametrize("bi", [False, True], ids=["forward", "bidirectional"])
def test_stream_restart_on_poisoned_state_matches_a_fresh_stream(params, bi, warm, pattern):
    """A sequence, reset(), then -- at that clean point -- the stream's whole state poisoned (its own Workspace, fn, fn_split,
    flow_low, init, scratch, the cn_* slots, the encoders' sets) and a DIFFERENT sequence: every output, masks and residuals
    included, is a fresh stream's on a fresh model.  Half way through that sequence the stream is poisoned once more, now as a
    RUNNING stream (clean=False): all but what it carries to the next call -- the cached frame, the last flow."""
    want = stream_ref(params, warm, bi)
    m = build(params, "bf16x3")
    s = make_stream(m, warm, bi)
    with torch.no_grad():
        first = [s(f) for f in frames(5, (1, 3))]
        assert first[0] is None and all(o is not None for o in first[1:])
        s.reset()
        a = model_audit(m, ("stream", s._st))
        snap = sa.snapshot(a)
        assert sa.poison(a, pattern) > 0
        assert_poisoned(a, ["stream.fn", "stream.fn_split", "stream.flow_low", "stream.init", "stream.scratch", "stream.ws.net0_ab",
                            "stream.ws.f_all", "stream.ws.img_c", "stream.ws.pyr_a[0]"] +
                        (["stream.fi_in", "stream.cn_net[0]", "stream.cn_net_s[1]", "stream.cn_x_s[0]"] if bi else []))
        tag = f"{'bidirectional' if bi else 'forward'} stream warm={warm}, poison {pattern}"
        problems = []
        for t, f in enumerate(frames(77, (2, -5))):
            if t == 2:
                running = model_audit(m, ("stream", s._st), clean=False)
                assert sa.poison(running, pattern) > 0
                assert_poisoned(running, ["stream.fn", "stream.init", "stream.ws.net0_ab"] + ([] if bi else ["stream.ws.f_all"]))
                assert bool(torch.isfinite(s._st.flow_low).all()) and float(s._st.flow_low.abs().max()) < 1e3
            problems.append(mismatch(s(f), want[t], f"{tag}, frame {t}"))
        assert len(want[0]) == 0 and len(want[1]) == (6 if bi else 1)
        conclude(problems, model_audit(m, ("stream", s._st), clean=False), snap)
        # the snapshot was taken after the first sequence: the constants are also those of a workspace just constructed
        ws = s._st.ws
        new = type(ws)(m._lib(), ws.B, ws.H, ws.W, ws.device, f16=ws.f16, alt_corr=ws.alt_corr)
        for k in ("g_a2b", "g_a2b_8", "g_b2a_8", "g_a2b_8_il", "g_b2a_8_il", "coords0"):
            assert torch.equal(getattr(ws, k), getattr(new, k)), k


# ---- (d) training buffers --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rig(params):
    """As tests/test_hip_train_loop.py's: a PriOr_RAFT in train() + freeze_bn() and its flat optimizer (never stepped)."""
    from prior_flow_amd import train as tr
    m = build(params, "bf16x3").train()
    m.freeze_bn()
    opt, _ = tr.fetch_optimizer(argparse.Namespace(lr=1e-4, wdecay=5e-5, epsilon=1e-8, num_steps=1000, clip=1.0), m)
    return m, opt


@pytest.mark.parametrize("pattern", sa.PATTERNS)
def test_training_step_on_poisoned_loop_buffers(rig, pattern, monkeypatch):
    """tests/test_hip_train_loop.py's harness and shape.  Steps on one input set (the second one allocates the gradient sink's
    arena), then LoopBuffers' SCRATCH cells and the arena poisoned, then a step on a second set: its forward predictions are, bit
    for bit, those of a loop whose buffers were just allocated; its gradients -- accumulated with fp32 atomics, so not
    reproducible bitwise -- meet the float64 reference within the per-parameter bounds of tests/train_loop_ref.py, through the
    same functions as test_loop_backward_is_the_vjp_at_its_saved_state; d_delta[..., 2:4] and d_out's dead columns stay zero."""
    import test_hip_train_loop as thl
    import train_loop_ref as tl
    from prior_flow_amd.autograd import SINK
    thl._schedule(monkeypatch, "1")
    case, first, second = tl.EVEN, thl._inputs(tl.EVEN), thl._inputs(tl.EVEN_B)
    m, opt = rig
    with tl.clean_tape():
        m._loop_bufs = None                             # a fresh loop: the reference of the forward
        h = tl.Harness(m, opt, case)
        h.load(second)
        h.step(True)
        want = [p.detach().clone() for p in h.preds]
        m._loop_bufs = None
        h = tl.Harness(m, opt, case)
        for _ in range(2):
            h.load(first)
            h.step(True)
        sink = SINK.for_device(h.dev.index)
        assert sink.arena is not None and sink.arena.numel() > 0
        h.forget()
        h.load(second)                                  # (zeroes the loop's buffers: the poison goes in behind it)
        a = sa.audit(("loop", m._loop_bufs))
        snap = sa.snapshot(a)
        assert sa.poison(a, pattern) > 0
        sink.arena.copy_(sa.pattern_like(sink.arena, pattern))
        h.step(True)
        line, epe, fails, preds = thl._compare(h, case, second, f"{case.name} after poison {pattern}")
        conclude([mismatch(preds, want, f"training step after poison {pattern}")], sa.audit(("loop", m._loop_bufs)), snap)
        thl._assert_close(line, epe, fails)
