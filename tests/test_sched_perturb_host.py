"""What tests/sched_perturb.py rests on, without a GPU: (1) every launch of the library takes its queue from PfLib._stream() --
statically, from include/priorflow_hip.h and _lib.py's AST; (2) the harness's bookkeeping, on the host emulation library with
injected queue ids; (3) the claim that a delay of d >= T in front of every launch of one queue makes every missing cross-queue
edge lose, as a discrete-event simulation over random schedules."""
import ast
import os
import random
import re

import pytest
import torch

import sched_perturb as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "prior-flow_amd")
AUDITED_DIRECT = {("debug_dirty_lds", "pf_debug_dirty_lds")}       # the one launch whose handle is built beside _stream()


# ---- (1) the choke point ----------------------------------------------------------------------------------------------------------
def stream_params():
    """symbol -> (index of its `stream` parameter, number of parameters), for the declarations that have one."""
    text = open(os.path.join(ROOT, "include", "priorflow_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    out = {}
    for name, params in re.findall(r"\b(pf_[a-z0-9_]+)\s*\(([^;{}()]*)\)\s*;", text, flags=re.S):
        names = [re.findall(r"[A-Za-z_][A-Za-z0-9_]*", p)[-1] for p in params.split(",") if p.strip() and p.strip() != "void"]
        if "stream" in names:
            out[name] = (names.index("stream"), len(names))
    return out


def _is_dll(node):
    return isinstance(node, ast.Attribute) and node.attr == "_dll"


def uncovered(source, streams):
    """(problems, sites): every X._dll.pf_* call (direct or through getattr) of `source` whose symbol has a stream parameter and
    whose argument there is not `<lib>._stream(...)`, by function and symbol; and the number of call sites that were checked."""
    tree = ast.parse(source)
    problems, sites = [], 0
    for fn in [n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef)]:
        own = [n for n in ast.walk(fn)]
        inner = {id(m) for sub in own if isinstance(sub, ast.FunctionDef) and sub is not fn for m in ast.walk(sub)}
        strings = {}                                                # local name -> the "pf_*" constants assigned to it
        for n in own:
            if isinstance(n, ast.Assign) and len(n.targets) == 1 and isinstance(n.targets[0], ast.Name):
                strings.setdefault(n.targets[0].id, []).extend(
                    c.value for c in ast.walk(n.value) if isinstance(c, ast.Constant) and isinstance(c.value, str) and c.value.startswith("pf_"))
        for call in own:
            if id(call) in inner or not isinstance(call, ast.Call):
                continue
            f = call.func
            if isinstance(f, ast.Attribute) and f.attr.startswith("pf_") and _is_dll(f.value):
                symbols = [f.attr]
            elif (isinstance(f, ast.Call) and isinstance(f.func, ast.Name) and f.func.id == "getattr" and len(f.args) == 2
                  and _is_dll(f.args[0])):
                a = f.args[1]
                symbols = [a.value] if isinstance(a, ast.Constant) else strings.get(getattr(a, "id", None), [])
                if not symbols:
                    problems.append(f"{fn.name}: getattr(_dll, ...) at line {call.lineno} with a name this check cannot resolve")
                    continue
            else:
                continue
            for sym in symbols:
                if sym not in streams:
                    continue
                sites += 1
                idx, n = streams[sym]
                plain = not call.keywords and not any(isinstance(a, ast.Starred) for a in call.args)
                assert plain or idx == n - 1, sym                   # (behind a *args the stream is found as the last argument)
                arg = (call.args[idx] if plain and idx < len(call.args) else call.args[-1]) if call.args else None
                ok = isinstance(arg, ast.Call) and isinstance(arg.func, ast.Attribute) and arg.func.attr == "_stream"
                if not ok and (fn.name, sym) in AUDITED_DIRECT and isinstance(arg, ast.Name):
                    ok = True
                if not ok:
                    problems.append(f"{fn.name}: {sym} (line {call.lineno}) does not take its stream from _stream()")
    return problems, sites


def test_every_launch_takes_its_queue_from_the_choke_point():
    """Every self._dll.pf_* call whose header entry has a `stream` parameter passes self._stream(...) there, or is the audited
    direct site; no other module of the package touches the library handle or a raw queue handle.  What Perturb patches is
    therefore what every launch goes through."""
    streams = stream_params()
    assert len(streams) >= 90 and "pf_conv2d" in streams and "pf_conv2d_tile" not in streams, len(streams)
    src = open(os.path.join(PKG, "_lib.py")).read()
    problems, sites = uncovered(src, streams)
    assert not problems, "\n".join(problems)
    assert sites >= 96, sites
    # a raw handle is built in two places only: _stream() itself and the audited site
    tree = ast.parse(src)
    raw = sorted({fn.name for fn in ast.walk(tree) if isinstance(fn, ast.FunctionDef)
                  for n in ast.walk(fn) if isinstance(n, ast.Attribute) and n.attr == "cuda_stream"})
    assert raw == ["_stream", "debug_dirty_lds"], raw
    for f in sorted(os.listdir(PKG)):
        if f.endswith(".py") and f != "_lib.py":
            text = open(os.path.join(PKG, f)).read()
            assert "._dll" not in text and "cuda_stream" not in text, f


def test_the_coverage_check_names_a_hand_built_handle():
    """The check has teeth: one _stream( replaced by a hand-built handle in a copy of the source is reported by name -- a direct
    call, a getattr call and the audited site's name on another function."""
    streams = stream_params()
    src = open(os.path.join(PKG, "_lib.py")).read()
    hand = "C.c_void_p(torch.cuda.current_stream().cuda_stream)"
    for old, fn, sym in (("x.numel(), self._stream(x)), \"pf_add_relu\")", "add_relu", "pf_add_relu"),
                         ("B, H8, W8, self._stream(x)), fn)", "conf_stem", "pf_conf_stem"),
                         ("len(descs), B, H8, W8, self._stream(like)), \"pf_conv2d\")", "conv2d", "pf_conv2d")):
        assert src.count(old) == 1, old
        problems, _ = uncovered(src.replace(old, old.replace(re.search(r"self\._stream\(\w+\)", old).group(0), hand)), streams)
        assert problems and all(p.startswith(f"{fn}: ") for p in problems) and any(sym in p for p in problems), (fn, problems)
    moved = src.replace("self._stream(x)), \"pf_add_relu\")", "stream), \"pf_add_relu\")")
    got = uncovered(moved, streams)[0]          # a plain name is accepted at the audited site only
    assert len(got) == 1 and got[0].startswith("add_relu: pf_add_relu (line ") and got[0].endswith("does not take its stream from _stream()")


# ---- (2) bookkeeping --------------------------------------------------------------------------------------------------------------
class Queues:
    """An injected 'current queue' for the emulation library, where there are no streams."""

    def __init__(self):
        self.cur, self.alias = 0x10, {}

    def __call__(self, device=None):
        return self.alias.get(self.cur, self.cur)


def _toy(lib, q, x, y, out):
    """Seven launches on three fake queues; two of them are torch ops."""
    q.cur = 0x10
    lib.add_relu(x, y, out)                 # 0
    q.cur = 0x20
    lib.relu_mask(x, y, out)                # 1
    torch.add(x, y, out=out)                # 2  (a torch-native op inside the schedule)
    q.cur = 0x10
    lib.add_relu(x, y, out)                 # 3
    out.view(-1)[:4]                        #    views launch nothing
    q.cur = 0x30
    out.copy_(x)                            # 4
    q.cur = 0x20
    lib.add_relu(x, y, out)                 # 5
    q.cur = 0x10
    lib.relu_mask(x, y, out)                # 6
    return out


def test_launch_log_counts_victims_and_blocks():
    import emu_lib
    lib = emu_lib.load()
    q = Queues()
    x, y, out = torch.randn(64), torch.randn(64), torch.empty(64)
    fired = []

    def delay():
        fired.append(q.cur)
        torch.zeros(4).add_(1.0)            # the delay's own op is neither logged nor delayed

    with sp.Perturb(queue_of=q, devices=("cpu",)) as dry:
        _toy(lib, q, x, y, out)
    assert [(n, m, h) for n, m, h in dry.log] == [
        (0, "add_relu", 0x10), (1, "relu_mask", 0x20), (2, "aten.add.out", 0x20), (3, "add_relu", 0x10), (4, "aten.copy_.default", 0x30),
        (5, "add_relu", 0x20), (6, "relu_mask", 0x10)]
    assert list(dry.counts().items()) == [(0x10, 3), (0x20, 3), (0x30, 1)] and dry.injected == [] and not fired
    want = out.clone()
    # a victim by handle: a delay in front of each of its launches, torch ops included, and nowhere else
    with sp.Perturb(victim=0x20, delay=delay, queue_of=q, devices=("cpu",)) as p:
        _toy(lib, q, x, y, out)
    assert p.injected == [1, 2, 5] and fired == [0x20] * 3 and p.log == dry.log and torch.equal(out, want)
    # ... by a predicate over handles
    del fired[:]
    with sp.Perturb(victim=lambda h: h > 0x20, delay=delay, queue_of=q, devices=("cpu",)) as p:
        _toy(lib, q, x, y, out)
    assert p.injected == [4] and fired == [0x30]
    # ... a block of ordinals
    del fired[:]
    with sp.Perturb(victim=0x10, block=range(3, 7), delay=delay, queue_of=q, devices=("cpu",)) as p:
        _toy(lib, q, x, y, out)
    assert p.injected == [3, 6] and fired == [0x10] * 2
    # a queue nobody launches on: nothing injected (run_perturbed asserts a nonzero count for that reason)
    with sp.Perturb(victim=0x99, delay=delay, queue_of=q, devices=("cpu",)) as p:
        _toy(lib, q, x, y, out)
    assert p.injected == [] and len(p.log) == 7
    # the patches are gone
    from prior_flow_amd._lib import PfLib
    assert PfLib._stream.__name__ == "_stream" and PfLib._stream.__qualname__.startswith("PfLib.")
    n = len(p.log)
    lib.add_relu(x, y, out)
    assert len(p.log) == n


def test_run_perturbed_cycles_the_victims_and_counts_the_delays(capsys):
    """run_perturbed on the emulation: one run per queue (two for a queue split into blocks), each with exactly that queue's
    launches delayed; a result that differs under one victim is reported with the victim and its launch count."""
    import emu_lib
    lib = emu_lib.load()
    q = Queues()
    x, y, out = torch.randn(64), torch.randn(64), torch.empty(64)
    fired, decoys = [], []

    def delay():
        fired.append(q.cur)

    def mismatch(got, want, what):
        return None if torch.equal(got, want) else f"{what}: output 0 differs"

    want = _toy(lib, q, x, y, out).clone()
    lines = sp.run_perturbed(lambda: _toy(lib, q, x, y, out), lambda: decoys.append(1), want, mismatch, "toy", delay=delay,
                             blocks={"#0": 2}, sync=lambda: None, queue_of=q, devices=("cpu",))
    assert lines == [] and len(decoys) == 5                     # dry + 2 blocks of queue #0 + queues #1, #2
    assert fired == [0x10] + [0x10] * 2 + [0x20] * 3 + [0x30]
    assert "[sched] toy: 7 launches on 3 queues: #0 0x10 x3, #1 0x20 x3, #2 0x30 x1" in capsys.readouterr().out

    wrong = want + 1

    def racy():                                                 # wrong whenever queue 0x20 has been delayed
        r = _toy(lib, q, x, y, out)
        return wrong if fired and fired[-1] == 0x20 else r
    lines = sp.run_perturbed(racy, lambda: None, want, mismatch, "toy", delay=delay, sync=lambda: None, queue_of=q, devices=("cpu",))
    assert len(lines) == 1 and "victim queue #1 (0x20, 3 launches) delayed" in lines[0]
    # queues by name: what is not named is the queue "other"; a block is a contiguous range of ordinals
    del fired[:]
    lines = sp.run_perturbed(lambda: _toy(lib, q, x, y, out), lambda: None, want, mismatch, "toy", delay=delay, sync=lambda: None,
                             roles={"main": 0x10, "late": lambda: 0x30}, blocks={"main": 3}, queue_of=q, devices=("cpu",))
    assert lines == [] and fired == [0x10] * 3 + [0x30] + [0x20] * 3
    assert "main 0x10 x3, late 0x30 x1, other 0x20 x3" in capsys.readouterr().out
    # one part of the log per case: ordinals 0..2 and 3..6; a queue without launches in the part is not run
    for part, want_fired in ((0, [0x10] + [0x20] * 2), (1, [0x10] * 2 + [0x20] + [0x30])):
        del fired[:]
        assert sp.run_perturbed(lambda: _toy(lib, q, x, y, out), lambda: None, want, mismatch, "toy", delay=delay, sync=lambda: None,
                                window=(part, 2), queue_of=q, devices=("cpu",)) == []
        assert fired == want_fired, (part, fired)


def test_a_run_whose_fresh_stream_takes_a_named_handle_is_repeated(capsys):
    """A call that creates a stream of its own per run (a graph capture's warm-up stream) now and then gets one whose handle is a
    named queue's; its launches would then count as that queue's.  Such a run is repeated, so every victim's run delays exactly
    the launches the settled dry run gave that queue."""
    import emu_lib
    lib = emu_lib.load()
    q = Queues()
    x, y, out = torch.randn(64), torch.randn(64), torch.empty(64)
    fired, runs = [], []

    def fresh():
        runs.append(1)
        q.alias = {0x30: 0x20} if len(runs) == 3 else {}        # the third run's own stream coincides with the named 0x20

    want = _toy(lib, q, x, y, out).clone()
    lines = sp.run_perturbed(lambda: _toy(lib, q, x, y, out), lambda: None, want, lambda g, w, what: None if torch.equal(g, w) else what,
                             "toy", delay=lambda: fired.append(q.cur), sync=lambda: None, roles={"main": 0x10, "side": 0x20},
                             fresh=fresh, queue_of=q, devices=("cpu",))
    assert lines == [] and len(runs) == 6                       # two dry runs that agree, main twice, side, other
    assert fired == [0x10] * 3 + [0x10] * 3 + [0x20] * 3 + [0x30]
    text = capsys.readouterr().out
    assert "main 0x10 x3, side 0x20 x3, other 0x30 x1" in text and text.count("repeated") == 1


class _FakeEvent:
    def __init__(self):
        self.on = None

    def record(self, stream):
        self.on = stream

    def wait(self, stream):
        stream.waited.append(self.on.cuda_stream)


class _FakeStream:
    """torch.cuda.Stream's Python layer (wait_stream is wait_event(record_event())) over a list."""

    def __init__(self, h):
        self.cuda_stream, self.waited = h, []

    def wait_event(self, event):
        event.wait(self)

    def record_event(self):
        e = _FakeEvent()
        e.record(self)
        return e

    def wait_stream(self, stream):
        self.wait_event(stream.record_event())


def _schedule(a, b, c):
    ev = _FakeEvent()
    ev.record(a)
    b.wait_event(ev)            # 0: recorded on a
    c.wait_stream(b)            # 1: one wait, although wait_stream is record_event + wait_event
    ev2 = _FakeEvent()
    ev2.record(c)
    a.wait_event(ev2)           # 2: recorded on c
    a.wait_stream(b)            # 3


def test_drop_wait_skips_one_wait_and_names_the_recording_queue(monkeypatch):
    monkeypatch.setattr(torch.cuda, "Stream", _FakeStream)
    monkeypatch.setattr(torch.cuda, "Event", _FakeEvent)
    orig = (_FakeStream.wait_event, _FakeStream.wait_stream, _FakeEvent.record)
    mk = lambda: (_FakeStream(0xa), _FakeStream(0xb), _FakeStream(0xc))  # noqa: E731
    a, b, c = mk()
    with sp.DropWait() as dry:
        _schedule(a, b, c)
    assert [(k, fn, j, w, r) for k, fn, j, _, w, r in dry.waits] == [
        (0, "_schedule", 0, 0xb, 0xa), (1, "_schedule", 1, 0xc, 0xb), (2, "_schedule", 2, 0xa, 0xc), (3, "_schedule", 3, 0xa, 0xb)]
    assert dry.dropped is None and (a.waited, b.waited, c.waited) == ([0xc, 0xb], [0xa], [0xb])
    assert len({line for _, _, _, line, _, _ in dry.waits}) == 4
    for k, left in ((0, ([0xc, 0xb], [], [0xb])), (1, ([0xc, 0xb], [0xa], [])), (2, ([0xb], [0xa], [0xb])), (3, ([0xc], [0xa], [0xb]))):
        a, b, c = mk()
        with sp.DropWait(k) as dw:
            _schedule(a, b, c)
        assert (a.waited, b.waited, c.waited) == left, k
        assert dw.dropped == dry.waits[k] and len(dw.waits) == 4
    assert (_FakeStream.wait_event, _FakeStream.wait_stream, _FakeEvent.record) == orig


# ---- (3) d >= T ---------------------------------------------------------------------------------------------------------------------
def simulate(queue, dur, waits, victim=None, d=0.0):
    """In-order queues, launches issued in list order by a host that never blocks; waits[i]: launches (on other queues, issued
    earlier) whose completion launch i's queue is made to wait for just before i is issued.  A delay is an item of its own on the
    victim's queue, in front of the launch and behind the launch's waits.  Returns (start, end)."""
    qend, start, end = {}, [], []
    for i, q in enumerate(queue):
        t = max([qend.get(q, 0.0)] + [end[j] for j in waits[i]])
        if q == victim:
            t += d
        start.append(t)
        end.append(t + dur[i])
        qend[q] = end[i]
    return start, end


def _implied(queue, waits, p, c):
    """Is p -> c ordered by queue order and the edges in `waits`?"""
    succ = {}
    last = {}
    for i, q in enumerate(queue):
        if q in last:
            succ.setdefault(last[q], []).append(i)
        last[q] = i
        for j in waits[i]:
            succ.setdefault(j, []).append(i)
    seen, todo = {p}, [p]
    while todo:
        for n in succ.get(todo.pop(), ()):
            if n == c:
                return True
            if n not in seen:
                seen.add(n)
                todo.append(n)
    return False


def random_schedule(rng):
    """2-5 queues, 20-60 launches with durations, record/wait edges forming a DAG (an edge always points to a later launch), and
    one LOAD-BEARING edge taken out: (queue, dur, waits without it, producer, consumer)."""
    while True:
        nq, n = rng.randint(2, 5), rng.randint(20, 60)
        queue = [rng.randrange(nq) for _ in range(n)]
        dur = [rng.choice((0.2, 1.0, 1.0, 3.0, 10.0)) * rng.uniform(0.5, 1.5) for _ in range(n)]
        waits = [[] for _ in range(n)]
        for i in range(1, n):
            for _ in range(rng.choice((0, 0, 1, 1, 2))):
                j = rng.randrange(i)
                if queue[j] != queue[i] and j not in waits[i]:
                    waits[i].append(j)
        edges = [(j, i) for i in range(n) for j in waits[i]]
        rng.shuffle(edges)
        for p, c in edges:
            cut = [[j for j in w if (j, i) != (p, c)] for i, w in enumerate(waits)]
            if not _implied(queue, cut, p, c):                  # nothing else orders the pair: the edge carries it
                return queue, dur, cut, p, c


def test_a_delay_of_T_exposes_every_missing_edge_in_random_schedules():
    """The claim behind the harness.  300 random schedules, each with one load-bearing edge P -> C removed (P writes what C reads;
    or P reads what C overwrites -- the ordering requirement is the same).  With the delay rule on P's queue and d = T, the
    undelayed duration of the schedule as it stands, C starts before P has ended in EVERY one; with d = 0 a share stays hidden
    (C starts behind P's end by luck), which is what the suite's passive screens see."""
    rng = random.Random(20240611)
    hidden = exposed = 0
    N = 300
    for _ in range(N):
        queue, dur, waits, p, c = random_schedule(rng)
        start, end = simulate(queue, dur, waits)
        T = max(end)
        hidden += start[c] >= end[p]
        s, e = simulate(queue, dur, waits, victim=queue[p], d=T)
        exposed += s[c] < e[p]
        # the intact schedule keeps the order under the same delays (the harness invents nothing)
        full = [w + [p] if i == c else w for i, w in enumerate(waits)]
        for v in set(queue):
            s, e = simulate(queue, dur, full, victim=v, d=T)
            assert all(s[i] >= e[j] for i, w in enumerate(full) for j in w)
    print(f"[sched] simulation: {hidden} of {N} missing edges stay hidden at d = 0 ({100.0 * hidden / N:.1f} %), "
          f"{N - exposed} of {N} at d = T")
    assert hidden > 0, "no schedule hides its missing edge undelayed: the simulation proves nothing"
    assert exposed == N
