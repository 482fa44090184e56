"""Cross-queue ordering, tested actively: one queue at a time is delayed in front of every launch it receives (helper; nothing
here is collected).

The launch schedules spread one call over several queues and tie them together with Event.record / wait_event / wait_stream.
A consumer that lacks its edge normally still runs behind its producer, by luck; the suite's bitwise screens then pass.  Here
the luck is taken away.  Every HIP launch takes its queue from PfLib._stream() (and debug_dirty_lds' one direct handle;
tests/test_sched_perturb_host.py proves that statically), every torch-native device op passes a TorchDispatchMode -- so for one
call under test:

  1. a dry run logs (ordinal, issuing method, queue) of every launch and lists the queues with their launch counts;
  2. per queue (the VICTIM) the call is repeated with a delay enqueued on the victim in front of every launch and torch op
     issued to it, and on no other queue;
  3. the result has to equal the reference bit for bit.

Why that suffices.  Producer P on the victim, consumer C elsewhere, no edge between them.  Undelayed, C started a margin
m >= 0 behind P's end.  Delays in front of P's predecessors move C by at most what they move P; the delay directly in front of
P moves P alone, so the race is lost when d > m, and m is at most the undelayed duration T of the whole call: d >= T suffices.
The same holds for a write-after-read pair when the READER's queue is the victim, so cycling the victim over all queues covers
both kinds in both directions (the discrete-event simulation in the host tests checks the claim on random schedules).

What a premature reader finds is another valid problem's data: in front of every perturbed run the same object runs an undelayed
call on a DIFFERENT input (the decoy) and the host synchronises.  Never NaN or +-1e30 (state_audit.poison): a race that is
FORCED to lose would certainly feed such values to a lookup as coordinates.

Limit: torch streams share a few hardware queues, and two streams on one hardware queue serialise.  A race between them cannot
be shown -- that can hide a defect, never invent one.

A queue is identified by its handle.  Where a call creates streams of its own whose handles differ from run to run (the warm-up
stream of a graph capture), run_perturbed takes the known queues by name (``roles=``) and treats every other handle as one more
queue, "other".

Torch streams map onto a few hardware queues, so concurrent_streams() picks streams that demonstrably overlap pairwise; the
schedules under test are given those (the caller's stream and the model's three side streams)."""
import json
import math
import os
import statistics
import sys
import time
from collections import OrderedDict

import torch
from torch.utils._python_dispatch import TorchDispatchMode

# torch ops that enqueue nothing: allocations and aliases
_NO_LAUNCH = {"aten.empty_like.default", "aten.new_empty.default", "aten.new_empty_strided.default", "aten.empty_strided.default",
              "aten.detach.default", "aten.alias.default", "aten.lift_fresh.default", "aten.new_zeros.default"}


def current_queue(device=None):
    return int(torch.cuda.current_stream(device).cuda_stream)


class Delay:
    """`passes` in-place passes over a private buffer on the current stream: plain capturable torch ops, in the style of _busy
    in tests/test_hip_augment.py.  The buffer is allocated here -- in front of any capture -- and touched by nothing else."""

    def __init__(self, mbytes=1024, passes=1, device="cuda"):
        self.buf = torch.ones(mbytes << 18, dtype=torch.float32, device=device)
        self.passes = passes

    def __call__(self):
        for _ in range(self.passes):
            self.buf.mul_(1.0)

    def device_ms(self, repeat=5):
        """One delay on an idle device, by device events: the median of `repeat`."""
        ms = []
        for _ in range(repeat):
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            self()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return statistics.median(ms)


class _Mode(TorchDispatchMode):
    def __init__(self, owner):
        super().__init__()
        self.owner = owner

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        o = self.owner
        if not o._busy:
            dev = o._device_of(args, kwargs)
            if dev is not None and not getattr(func, "is_view", False) and str(func) not in _NO_LAUNCH:
                o._launch(str(func), dev)
        return func(*args, **kwargs)


class Perturb:
    """Context manager: logs every launch as (ordinal, issuing method, queue) and, with a delay, enqueues it on the victim's queue
    in front of every launch (or of those whose ordinal lies in `block`) that goes there.

    victim  the queue's handle (torch.cuda.Stream.cuda_stream), or a predicate over handles;
    block   a container of ordinals (a range), or None for all;
    delay   a callable that enqueues the delay on the current stream (Delay); None: a dry run.
    queue_of / devices: what names the current queue and which tensors count as device tensors (the host tests inject fake queue
    ids under the emulation library)."""

    def __init__(self, victim=None, block=None, delay=None, queue_of=current_queue, devices=("cuda",)):
        self.victim, self.block, self.delay = victim, block, delay
        self.queue_of, self.devices = queue_of, tuple(devices)
        self.log = []               # (ordinal, issuing method, queue handle)
        self.injected = []          # ordinals that got a delay
        self.ranks = OrderedDict()  # queue handle -> rank
        self._busy = False

    # ---- bookkeeping --------------------------------------------------------------------------------------------------------
    def _device_of(self, args, kwargs):
        for a in list(args) + list(kwargs.values()):
            for t in (a if isinstance(a, (list, tuple)) else (a,)):
                if isinstance(t, torch.Tensor) and t.device.type in self.devices:
                    return t.device
        return None

    def _launch(self, method, device=None):
        q = self.queue_of(device)
        n = len(self.log)
        self.ranks.setdefault(q, len(self.ranks))
        self.log.append((n, method, q))
        hit = self.victim(q) if callable(self.victim) else (self.victim is not None and q == self.victim)
        if hit and self.delay is not None and (self.block is None or n in self.block):
            self._busy = True       # the delay's own ops are neither logged nor delayed
            try:
                self.delay()
            finally:
                self._busy = False
            self.injected.append(n)

    def counts(self):
        """queue handle -> number of launches, in the order of first launches."""
        c = OrderedDict((q, 0) for q in self.ranks)
        for _, _, q in self.log:
            c[q] += 1
        return c

    # ---- patches ------------------------------------------------------------------------------------------------------------
    def __enter__(self):
        from prior_flow_amd._lib import PfLib
        me = self
        self._orig = (PfLib._stream, PfLib.debug_dirty_lds)
        orig_stream, orig_dirty = self._orig

        def _stream(lib, t):
            if not me._busy:
                me._launch(sys._getframe(1).f_code.co_name, t.device if t.device.type in me.devices else None)
            return orig_stream(lib, t)

        def debug_dirty_lds(lib, pattern=0x7fc00000, like=None):
            if like is None and not me._busy:       # the one launch whose handle is not _stream()'s
                me._launch("debug_dirty_lds", None)
            return orig_dirty(lib, pattern, like)

        PfLib._stream, PfLib.debug_dirty_lds = _stream, debug_dirty_lds
        self._mode = _Mode(self)
        self._mode.__enter__()
        return self

    def __exit__(self, *exc):
        from prior_flow_amd._lib import PfLib
        self._mode.__exit__(*exc)
        PfLib._stream, PfLib.debug_dirty_lds = self._orig
        return False


class DropWait:
    """Context manager: counts the cross-queue waits a call executes (Stream.wait_event, Stream.wait_stream) and skips the k-th
    (k = None: none).  Event.record is followed so that a skipped wait can be attributed to the queue that recorded its event;
    for wait_stream(s) that queue is s.  `waits` lists (k, function, ordinal within that function, line, waiting queue,
    recording queue); `dropped` is the skipped one's entry."""

    def __init__(self, k=None):
        self.k = k
        self.waits, self.dropped = [], None
        self._recorded = {}         # id(event) -> (event, queue that recorded it)
        self._per_fn = {}
        self._inside = 0

    def _wait(self, frame, waiter, recorder):
        fn = frame.f_code.co_name
        j = self._per_fn[fn] = self._per_fn.get(fn, -1) + 1
        entry = (len(self.waits), fn, j, frame.f_lineno, waiter, recorder)
        self.waits.append(entry)
        if entry[0] == self.k:
            self.dropped = entry
            return True
        return False

    def __enter__(self):
        S, E = torch.cuda.Stream, torch.cuda.Event
        me = self
        self._orig = (S.wait_event, S.wait_stream, E.record)
        wait_event, wait_stream, record = self._orig

        def p_record(ev, stream=None):
            if stream is None:
                stream = torch.cuda.current_stream()
            me._recorded[id(ev)] = (ev, int(stream.cuda_stream))
            return record(ev, stream)

        def p_wait_event(s, ev):
            if me._inside == 0 and me._wait(sys._getframe(1), int(s.cuda_stream), me._recorded.get(id(ev), (None, None))[1]):
                return None
            return wait_event(s, ev)

        def p_wait_stream(s, other):
            if me._wait(sys._getframe(1), int(s.cuda_stream), int(other.cuda_stream)):
                return None
            me._inside += 1         # (Stream.wait_stream is wait_event(record_event()): one wait, not two)
            try:
                return wait_stream(s, other)
            finally:
                me._inside -= 1

        S.wait_event, S.wait_stream, E.record = p_wait_event, p_wait_stream, p_record
        return self

    def __exit__(self, *exc):
        S, E = torch.cuda.Stream, torch.cuda.Event
        S.wait_event, S.wait_stream, E.record = self._orig
        return False


# ---- calibration ------------------------------------------------------------------------------------------------------------------
TABLE = []                          # one row per calibrated case (PRIORFLOW_SCHED_TABLE names the file they are written to)
FACTOR = 1.25                       # timer jitter on top of the bound d >= T
_DELAY = {}


def shared_delay(device="cuda"):
    """One buffer for the process (1 GiB: a pass of ~0.5 ms keeps the number of passes, and of graph nodes, small)."""
    if device not in _DELAY:
        _DELAY[device] = Delay(1024, 1, device)
    return _DELAY[device]


def calibrate(call, name, delay=None):
    """T: host wall time of the undelayed call between two synchronises, median of 3.  The delay's number of passes is chosen so
    that ONE delay, by device events (median of 5), lasts >= 1.25 T.  Returns the row (also appended to TABLE)."""
    delay = delay or shared_delay()
    ts = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    T = statistics.median(ts)
    delay.passes = 8
    per_pass = delay.device_ms() / 8
    delay.passes = max(1, math.ceil(FACTOR * T / per_pass))
    d = delay.device_ms()
    while d < FACTOR * T:
        delay.passes = delay.passes + max(1, delay.passes // 8)
        d = delay.device_ms()
    row = dict(case=name, T_ms=round(T, 4), T_runs_ms=[round(t, 4) for t in ts], passes=delay.passes, d_ms=round(d, 4),
               d_over_T=round(d / T, 3))
    TABLE.append(row)
    return row


def write_table():
    path = os.environ.get("PRIORFLOW_SCHED_TABLE")
    if path:
        with open(path, "w") as f:
            json.dump(dict(factor=FACTOR, note="T: host wall time of the undelayed eager call (median of 3); d: one delay by "
                                                "device events (median of 5); queues: launches per queue in order of first launch",
                           cases=TABLE), f, indent=1)


# ---- the experiment ---------------------------------------------------------------------------------------------------------------
def overlap(a, b, delay):
    """Does work on stream b demonstrably run while stream a is busy?  a: a delay, then flag = 1; b, with no edge: seen = flag.
    seen == 0 proves the overlap; two streams on one hardware queue serialise and give 1.  (Ordinary allocations: the race this
    provokes yields one of two valid values.)"""
    flag, seen = torch.zeros(1, device="cuda"), torch.ones(1, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(a):
        delay()
        flag.fill_(1.0)
    with torch.cuda.stream(b):
        seen.copy_(flag)
    torch.cuda.synchronize()
    return float(seen) == 0.0


def concurrent_streams(n, tries=16, delay=None):
    """n torch streams every two of which overlap in both directions (greedy over at most `tries` fresh streams), or None."""
    delay = delay or shared_delay()
    keep, delay.passes = delay.passes, 8
    try:
        chosen = []
        for _ in range(tries):
            s = torch.cuda.Stream()
            if all(s.cuda_stream != c.cuda_stream and overlap(s, c, delay) and overlap(c, s, delay) for c in chosen):
                chosen.append(s)
                if len(chosen) == n:
                    return chosen
        return None
    finally:
        delay.passes = keep


def run_perturbed(call, decoy, reference, mismatch, name, row=None, delay=None, roles=None, blocks=None, window=None,
                  fresh=None, sync=None, **how):
    """Dry run, then one perturbed run per victim queue; returns the mismatch lines (empty: every run gave `reference` bit for bit).

    call()      the call under test; returns its result (anything test_hip_state.flat understands)
    decoy()     an undelayed call of the same object on a different input, run (and synchronised) in front of every run
    mismatch    test_hip_state.mismatch
    row         the case's calibrate() row: the queues and counts are added to it
    roles       {name: handle, or a callable that returns it (None: not created yet)}: the queues by name; every other handle is
                the queue "other".  Default: the dry run's queues, "#0", "#1", ... in the order of their first launches
    blocks      {name: n}: that victim's launches are split into n contiguous blocks of ordinals, one perturbed run each
    window      (i, n): only the launches whose ordinal lies in the i-th of n contiguous parts of the whole log are delayed -- one
                test case per part keeps a long call's cases short; the derivation needs only the delay in front of P
    fresh()     called in front of every run (the dry run included) where the call needs a new object per run (a graph capture)
    how         further arguments of Perturb (queue_of, devices: the host tests)
    Per run: the launches are the dry run's, method by method and queue by queue; the delays sit in front of exactly the victim's
    launches (of its block), and their number is nonzero."""
    delay = delay or shared_delay()
    sync = sync or torch.cuda.synchronize

    def one(**kw):
        if fresh is not None:
            fresh()
        decoy()
        sync()
        with Perturb(**kw, **how) as p:
            out = call()
            sync()
        return p, out

    def role(q):
        for nm, h in roles.items():
            if q == (h() if callable(h) else h):
                return nm
        return "other"

    def handle(nm, p):
        hs = sorted({q for _, _, q in p.log if role(q) == nm})
        return "/".join(f"{h:#x}" for h in hs)

    def settled(want_roles=None, **kw):
        """One run whose launches went to the queues of `want_roles`.  A call that creates a stream of its own per run (fresh=)
        now and then gets one whose handle is a named queue's: that run is repeated with the next fresh object; the dry run is
        repeated until two in a row agree."""
        for _ in range(8):
            p, out = one(**kw)
            now = [role(q) for _, _, q in p.log]
            if want_roles is None and fresh is not None:
                want_roles = now
                continue
            if want_roles is None or now == want_roles:
                return p, out
            print(f"[sched] {name}: a fresh stream took a named queue's handle in this run: repeated")
            if not kw:
                want_roles = now
        raise AssertionError(f"{name}: the launches' queues changed in 8 runs in a row")

    if roles is None:
        dry, out = one()
        roles = OrderedDict((f"#{r}", q) for r, q in enumerate(dry.ranks))
    else:
        dry, out = settled()
    dry_roles = [role(q) for _, _, q in dry.log]
    names = [nm for nm in list(roles) + ["other"] if nm in dry_roles]
    assert names
    line = f"[sched] {name}: " + (f"T {row['T_ms']:.3f} ms, d {row['d_ms']:.3f} ms ({row['passes']} passes), " if row else "") + \
        f"{len(dry.log)} launches on {len(names)} queues: " + ", ".join(f"{nm} {handle(nm, dry)} x{dry_roles.count(nm)}" for nm in names)
    print(line)
    if row is not None:
        row["launches"] = len(dry.log)
        row["queues"] = {nm: dry_roles.count(nm) for nm in names}
    problems = [mismatch(out, reference, f"{name}, undelayed")]
    lo, hi = (0, len(dry.log)) if window is None else (window[0] * len(dry.log) // window[1], (window[0] + 1) * len(dry.log) // window[1])
    for nm in names:
        ords = [n for n, r in enumerate(dry_roles) if r == nm and lo <= n < hi]
        nb = (blocks or {}).get(nm, 1)
        for b in range(nb):
            part = ords[b * len(ords) // nb:(b + 1) * len(ords) // nb]
            if not part:
                continue
            first, last = part[0], part[-1]
            p, out = settled(dry_roles, victim=lambda q: role(q) == nm, delay=delay,
                             block=None if nb == 1 and window is None else range(first, last + 1))
            assert [m for _, m, _ in p.log] == [m for _, m, _ in dry.log], f"{name}: the perturbed run's launches are not the dry run's"
            assert p.injected == part and part, f"{name}: {len(p.injected)} delays for the {len(part)} launches of queue {nm}"
            problems.append(mismatch(out, reference, f"{name}, victim queue {nm} ({handle(nm, p)}, {len(ords)} launches"
                                     + (f", block {b + 1}/{nb}" if nb > 1 else "") + (f" of part {window[0] + 1}/{window[1]}" if window else "")
                                     + ") delayed"))
    return [p.replace("the call read resident state that it had not written -- bisect the poisoned set (module docstring)",
                      "a consumer ran before its producer (or a writer before its reader): a cross-queue edge is missing")
            for p in problems if p]
