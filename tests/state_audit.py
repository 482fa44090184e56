"""Audit of the product's RESIDENT device state (helper; nothing here is collected).

Every device buffer of the inference and training paths is allocated once with ``torch.zeros`` and reused for the life of the
model: ``engine.Workspace``, the buffer sets of both ``engine.EncoderPlan``s, ``video._StreamState`` / ``video._BiState`` and
``train_loop.LoopBuffers``.  This module enumerates those tensors, classifies every cell of every storage, and gives the tests

  * ``poison(audit, pattern)``: fill what a call may not rely on (class SCRATCH) with values that are loud when read;
  * ``snapshot(audit)`` / ``verify(audit, snap)``: check what must survive a call (classes CONST and ZERO).

Classes ("Resident state: what must survive a call and what may not"):

  CONST    written at construction and never again (the sample grids, coords0): bitwise unchanged.
  ZERO     must hold all-zero bits for ever: the K padding of the matrix-core operands and of the weight-gradient operands.
           The extents come from the allocation formulas of engine.split_twin / engine.f16_map, not from literals.
  SCRATCH  everything else: a call must overwrite whatever part of it the call reads.
  CARRIED  state a stream genuinely hands from one call to the next (the cached frame, flow_low).  It exists only when the audit
           is built with ``clean=False``; at a clean point -- a new stream, one after ``reset()`` -- the same cells are SCRATCH.
           (LoopBuffers is audited between steps only: between a forward and its backward all of it is carried.)

A tensor the enumeration finds and no rule classifies is an error that names it: a new buffer has to be classified here before
the suite passes.
"""
from __future__ import annotations

import re
from collections import OrderedDict
from typing import Callable, Dict, List, Optional, Tuple

import torch

CONST, ZERO, SCRATCH, CARRIED = "CONST", "ZERO", "SCRATCH", "CARRIED"

# attributes that hold no state of their own: captured graphs, and the references a stream keeps to the encoder plans' buffer
# sets so that its graphs' pointers stay valid (those sets are audited through the plans)
SKIP_ATTRS = ("graphs", "keep")

# the live input channels of update_block.encoder.conv: convc2's 192 + convf2's 64 (engine.py's layout comment, catB); its
# operand buffers are allocated with ODDC's geometry (272 = 128 + 64 + 64 + 16), the rest is zero padding of the K dimension
CAT_B_LIVE = 192 + 64


class AuditError(AssertionError):
    pass


# ---------------------------------------------------------------------------------------------------------------------------
# enumeration
# ---------------------------------------------------------------------------------------------------------------------------
def _ident(k) -> bool:
    return isinstance(k, str) and re.fullmatch(r"[A-Za-z_][A-Za-z_0-9]*", k) is not None


def _walk(v, name: str, out: list):
    if isinstance(v, torch.Tensor):
        out.append((name, v))
    elif isinstance(v, (list, tuple)):
        for i, x in enumerate(v):
            _walk(x, f"{name}[{i}]", out)
    elif isinstance(v, dict):
        for k, x in v.items():
            _walk(x, f"{name}.{k}" if _ident(k) else f"{name}[{k!r}]", out)


def named_tensors(obj, skip=SKIP_ATTRS) -> List[Tuple[str, torch.Tensor]]:
    """Every tensor reachable from ``vars(obj)`` (a dict: from its items) through lists, tuples and dicts, with its dotted name
    relative to `obj` (``net_a[1]``, ``pre[('a', '1')]``, ``a.d_delta``, ``act0[2]``).  Views are listed like any tensor."""
    out: list = []
    for k, v in (obj if isinstance(obj, dict) else vars(obj)).items():
        if k in skip:
            continue
        _walk(v, str(k), out)
    return out


def _covers_storage(t: torch.Tensor) -> bool:
    return t.is_contiguous() and t.storage_offset() == 0 and t.numel() * t.element_size() == t.untyped_storage().nbytes()


# ---------------------------------------------------------------------------------------------------------------------------
# rules: (holder, relative name, owner tensor) -> [(class, index into the owner, label)]; what no region claims is SCRATCH
# ---------------------------------------------------------------------------------------------------------------------------
class Rule:
    def __init__(self, fn: Callable, doc_class: str, doc: str):
        self.fn, self.doc_class, self.doc = fn, doc_class, doc


def _all(cls):
    return lambda holder, name, t: [(cls, (slice(None),) * t.dim(), "all")]


R_CONST = lambda doc: Rule(_all(CONST), CONST, doc)                                     # noqa: E731
R_SCRATCH = lambda doc="": Rule(lambda holder, name, t: [], SCRATCH, doc)               # noqa: E731


def R_COLS(lo: Optional[int], doc: str, live_of: Optional[Callable] = None):
    """ZERO: the columns (last dimension) from `lo` -- or from live_of(holder, name) -- to the end."""
    def fn(holder, name, t):
        a = lo if live_of is None else live_of(holder, name)
        return [(ZERO, (slice(None),) * (t.dim() - 1) + (slice(a, t.shape[-1]),), f"columns {a}..{t.shape[-1] - 1}")]
    return Rule(fn, ZERO, doc)


def operand_zero_regions(t: torch.Tensor, alloc: int, live: int):
    """The zero padding of a matrix-core operand buffer allocated for `alloc` channels of which `live` are ever written: a split
    twin bf16 [rows][(alloc + 31) // 32][2][32] (engine.split_twin) or an f16 map float16 [rows][(alloc + 63) // 64 * 64]
    (engine.f16_map).  The shapes are checked against those formulas."""
    if t.dtype == torch.bfloat16:
        chunks = (alloc + 31) // 32
        if t.dim() != 4 or tuple(t.shape[1:]) != (chunks, 2, 32):
            raise AuditError(f"split twin of {alloc} channels has shape {tuple(t.shape)}, expected [rows, {chunks}, 2, 32]")
        out = []
        full, rem = divmod(live, 32)
        if rem:
            out.append((ZERO, (slice(None), slice(full, full + 1), slice(None), slice(rem, 32)),
                        f"pad lanes {rem}..31 of chunk {full} (channels {live}..{full * 32 + 31})"))
            full += 1
        if full < chunks:
            out.append((ZERO, (slice(None), slice(full, chunks), slice(None), slice(None)), f"chunks {full}..{chunks - 1}"))
        return out
    if t.dtype == torch.float16:
        width = (alloc + 63) // 64 * 64
        if t.dim() != 2 or t.shape[1] != width:
            raise AuditError(f"f16 map of {alloc} channels has shape {tuple(t.shape)}, expected [rows, {width}]")
        return [(ZERO, (slice(None), slice(live, width)), f"columns {live}..{width - 1}")] if live < width else []
    raise AuditError(f"operand buffer of dtype {t.dtype}")


def _sibling(holder, name: str) -> torch.Tensor:
    """The fp32 buffer a twin mirrors: the same attribute without its ``_s`` (``net_a_s[1]`` -> ``net_a[1]``,
    ``xs1[0]`` / ``y1`` of an encoder set -> ``x1[0]``)."""
    m = re.fullmatch(r"(\w+?)(\[\d+\])?", name)
    base, idx = m.group(1), m.group(2)
    if isinstance(holder, dict):                        # encoder set: xs<l>[i], y<l> -> x<l>[0]
        return holder["x" + re.search(r"\d+", base).group(0)][0]
    v = getattr(holder, base[:-2])
    return v[int(idx[1:-1])] if idx and isinstance(v, (list, tuple)) else v


def R_TWIN(doc: str, live: Optional[int] = None):
    def fn(holder, name, t):
        alloc = _sibling(holder, name).shape[-1]
        return operand_zero_regions(t, alloc, alloc if live is None else live)
    return Rule(fn, ZERO, doc)


_S = R_SCRATCH
_TW = "K padding past the map's channels (none when the channels fill the last chunk)"

WORKSPACE_RULES: Dict[str, Rule] = OrderedDict(
    [(k, R_CONST("sample grid of the shape, written by pf_sample_grid at construction")) for k in
     ("g_a2b", "g_a2b_8", "g_b2a_8")] +
    [(k, R_CONST("the interleaved copy of a sample grid, made at construction")) for k in ("g_a2b_8_il", "g_b2a_8_il")] +
    [("coords0", R_CONST("the pixel grid, built at construction, copied into c1a / c1b per forward"))] +
    [(k, _S()) for k in
     ("f_all", "f_split", "img_c", "img_f", "pyr_a", "pyr_b", "feat_a", "feat_b", "c1a", "c1b", "flow_b", "flow_ba", "flow_tmp",
      "net0_ab", "x_ab", "net_a", "net_b", "z_a", "z_b", "rh_a", "rh_b", "own", "raw", "own_b", "raw_b", "corr_a", "corr_b",
      "c1_a", "c1_b", "cat_a", "flow4_a", "flow2_b", "t_a", "t_ba", "t_b", "conf_in", "conf_mid", "fh_a", "fh_b", "mh_a", "mh_b",
      "delta_a", "delta_b", "mask_a", "mask_b", "pre")] +
    [("cat_b", R_COLS(CAT_B_LIVE, "columns past update_block.encoder.conv's 256 inputs: K padding to conv_A's geometry"))] +
    [(k, R_TWIN(_TW)) for k in ("net0_ab_s", "net_a_s", "net_b_s", "x_ab_s", "rh_a_s", "rh_b_s", "c1_a_s", "c1_b_s", "cat_a_s",
                                "t_a_s", "t_ba_s", "t_b_s")] +
    [("cat_b_s", R_TWIN("everything past channel 255 (the twin's last chunk; an f16 map's columns 256..319)", live=CAT_B_LIVE))])

ENCODER_SET_RULES: Dict[str, Rule] = OrderedDict(
    [(k, _S()) for k in ("act", "s2d", "sc", "sh", "part", "x", "yr", "r")] +
    [(k, R_TWIN(_TW)) for k in ("xs", "y")])

_STREAM_COMMON = ("fn", "fn_split", "flow_low", "init", "scratch")
STREAM_RULES: Dict[str, Rule] = OrderedDict([(k, _S()) for k in _STREAM_COMMON])
BISTATE_RULES: Dict[str, Rule] = OrderedDict(
    [(k, _S()) for k in _STREAM_COMMON + ("fi_in", "cn_net", "cn_x")] +
    [(k, Rule(lambda holder, name, t: operand_zero_regions(t, 32 * t.shape[1], 32 * t.shape[1]), ZERO, _TW))
     for k in ("cn_net_s", "cn_x_s")])


def _loop_live(holder, name):           # d_out: conv_A has 124 outputs, update_block.encoder.conv 126 (x = [inp | out | flow tails])
    return {"a": 124, "b": 126}[name[0]]


LOOP_RULES: Dict[str, Rule] = OrderedDict(
    [(k, _S()) for k in
     ("corr", "c1", "cat", "x", "h", "h1", "z1", "z2", "rhr1", "rhr2", "q1", "q2", "fh", "mh", "mask", "delta", "c", "d_mask", "d_mh",
      "d_fh", "d_q1", "d_q2", "d_zr1", "d_zr2", "d_cat", "d_c1", "F", "dz", "d_corr", "d_raw", "d_flow", "own", "raw", "flow4", "t_a",
      "t_ba", "conf_in", "cf1", "d_t_a", "d_t_ba", "d_cf1", "d_conf", "flow_ba", "flow2", "t", "d_t")] +
    [("d_delta", R_COLS(2, "columns 2, 3: flow_head.conv2's 2 outputs padded to 4 (operand of its weight gradient)")),
     ("d_out", R_COLS(None, "columns past the 124 (A) / 126 (B) outputs of the motion encoder's last convolution", _loop_live))])

# the cells a running stream carries (only with clean=False)
def _carried_stream(st, relname, t):
    rows = st.rows
    if relname in ("flow_low",):
        return [(CARRIED, (slice(None),) * t.dim(), "the last pair's flow")]
    if relname in ("ws.img_c",):
        return [(CARRIED, (slice(None),) * t.dim(), "the cached frame's prepared images")]
    if relname in ("ws.f_all", "ws.f_split"):       # [f1A | f2A | f1B | f2B]: the first-frame slots
        return [(CARRIED, (slice(2 * v * rows, (2 * v + 1) * rows),) + (slice(None),) * (t.dim() - 1), f"view {v}, cached frame")
                for v in range(2)]
    return []


def _carried_bi(st, relname, t):
    if relname in ("flow_low", "ws.img_c", "ws.f_all", "ws.f_split") or relname.split("[")[0] in ("cn_net", "cn_x", "cn_net_s", "cn_x_s"):
        return [(CARRIED, (slice(None),) * t.dim(), "the cached frame")]
    return []


KINDS = {"Workspace": WORKSPACE_RULES, "_StreamState": STREAM_RULES, "_BiState": BISTATE_RULES, "LoopBuffers": LOOP_RULES,
         "EncoderSet": ENCODER_SET_RULES}


def _rule_key(kind: str, name: str) -> str:
    base = re.sub(r"\[[^\]]*\]", "", name)
    if kind == "LoopBuffers":
        return base.split(".", 1)[1] if "." in base else base
    if kind == "EncoderSet":
        return re.sub(r"\d+$", "", base)
    return base.split(".")[0]


# ---------------------------------------------------------------------------------------------------------------------------
# the audit
# ---------------------------------------------------------------------------------------------------------------------------
class Entry:
    """One storage: its owner tensor (the attribute that spans it), every name that reaches it, and its classified regions."""

    def __init__(self, name: str, owner: torch.Tensor):
        self.name, self.owner, self.aliases = name, owner, [name]
        self.regions: List[Tuple[str, tuple, str]] = []

    def scratch_mask(self) -> torch.Tensor:
        m = torch.ones(self.owner.shape, dtype=torch.bool, device=self.owner.device)
        for _cls, idx, _ in self.regions:
            m[idx] = False
        return m


class Audit:
    """``Audit().add(prefix, obj)`` for every container; `clean`: the state is at a clean point (see the module docstring)."""

    def __init__(self, clean: bool = True):
        self.clean = clean
        self.entries: "OrderedDict[int, Entry]" = OrderedDict()

    # -- building
    def add(self, prefix: str, obj, rules: Optional[Dict[str, Rule]] = None, kind: Optional[str] = None) -> "Audit":
        kind = kind or type(obj).__name__
        if kind == "EncoderPlan":
            for key, bset in obj._bufs_by_key.items():
                self.add(f"{prefix}{list(key)}", bset, kind="EncoderSet")
            return self
        if rules is None:
            if kind not in KINDS:
                raise AuditError(f"{prefix}: no classification table for a {kind}")
            rules = KINDS[kind]
        nested = [(k, v) for k, v in (obj.items() if isinstance(obj, dict) else vars(obj).items())
                  if type(v).__name__ in KINDS and not isinstance(v, (dict, list, tuple, torch.Tensor))]
        for k, v in nested:             # a stream's own Workspace, by the Workspace's table
            self.add(f"{prefix}.{k}", v)
        found = named_tensors(obj)
        # owners first: the attribute that spans a storage names it, whatever the order of the attributes
        for name, t in found:
            sid = t.untyped_storage().data_ptr()
            if t.numel() and sid not in self.entries and _covers_storage(t):
                self.entries[sid] = e = Entry(f"{prefix}.{name}", t)
                key = _rule_key(kind, name)
                if key not in rules:
                    raise AuditError(f"{e.name} (a {kind}'s `{key}`) is not classified: add it to tests/state_audit.py")
                self._classify(e, rules[key].fn(obj, name, t))
        for name, t in found:
            sid = t.untyped_storage().data_ptr()
            if not t.numel():
                continue
            if sid not in self.entries:
                raise AuditError(f"{prefix}.{name} is a view of a storage that no audited attribute spans")
            e = self.entries[sid]
            if f"{prefix}.{name}" not in e.aliases:
                e.aliases.append(f"{prefix}.{name}")
        if not self.clean:
            carried = {"_StreamState": _carried_stream, "_BiState": _carried_bi}.get(kind)
            if carried is None and kind not in ("EncoderSet", "Workspace"):
                raise AuditError(f"{prefix}: a {kind} is audited at a clean point only")
            for e in self.entries.values():
                if carried is not None and e.name.startswith(prefix + "."):
                    self._classify(e, carried(obj, e.name[len(prefix) + 1:], e.owner))
        return self

    def _classify(self, e: Entry, regions):
        """Adds regions to an entry: each in bounds, none overlapping another."""
        taken = ~e.scratch_mask()
        for cls, idx, label in regions:
            if len(idx) > e.owner.dim():
                raise AuditError(f"{e.name}: region {label} has {len(idx)} indices for {e.owner.dim()} dimensions")
            for d, s in enumerate(idx):
                if not (isinstance(s, slice) and s.step in (None, 1)):
                    raise AuditError(f"{e.name}: region {label}: only unit-step slices")
                lo, hi = (0 if s.start is None else s.start), (e.owner.shape[d] if s.stop is None else s.stop)
                if not 0 <= lo < hi <= e.owner.shape[d]:
                    raise AuditError(f"{e.name}: region {label} [{lo}:{hi}] is out of bounds of dimension {d} ({e.owner.shape[d]})")
            if bool(taken[idx].any()):
                raise AuditError(f"{e.name}: region {label} overlaps another region")
            taken[idx] = True
            e.regions.append((cls, idx, label))

    # -- queries
    def names(self) -> List[str]:
        return [e.name for e in self.entries.values()]

    def entry(self, name: str) -> Entry:
        for e in self.entries.values():
            if name == e.name or name in e.aliases:
                return e
        raise KeyError(name)

    def regions(self, cls: str):
        return [(e, idx, label) for e in self.entries.values() for c, idx, label in e.regions if c == cls]


def audit(*containers, clean: bool = True) -> Audit:
    """containers: (prefix, object) pairs -- Workspace, EncoderPlan, _StreamState, _BiState, LoopBuffers."""
    a = Audit(clean)
    for prefix, obj in containers:
        a.add(prefix, obj)
    return a


# ---------------------------------------------------------------------------------------------------------------------------
# poison
# ---------------------------------------------------------------------------------------------------------------------------
_INT_VIEW = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.float64: torch.int64,
             torch.int32: torch.int32}
# pattern `nan`: the quiet NaN of each format as bits; int32: -1
NAN_BITS = {torch.float32: 0x7fc00000, torch.float16: 0x7e00, torch.bfloat16: 0x7fc0, torch.float64: 0x7ff8000000000000,
            torch.int32: -1}
# pattern `big`: finite, +- alternating per element -- a ReLU turns a NaN into 0 (fmaxf(NaN, 0) = 0) but lets +big through
BIG = {torch.float32: 1e30, torch.float16: 6e4, torch.bfloat16: 1e30, torch.float64: 1e300, torch.int32: 0x7fffffff}
PATTERNS = ("nan", "big")


def pattern_like(t: torch.Tensor, pattern: str) -> torch.Tensor:
    if t.dtype not in _INT_VIEW:
        raise AuditError(f"no poison pattern for dtype {t.dtype}")
    if pattern == "nan":
        return torch.full(t.shape, NAN_BITS[t.dtype], dtype=_INT_VIEW[t.dtype], device=t.device).view(t.dtype)
    if pattern != "big":
        raise ValueError(pattern)
    p = torch.full((t.numel(),), BIG[t.dtype], dtype=t.dtype, device=t.device)
    if t.dtype.is_floating_point:
        p[1::2] = -BIG[t.dtype]
    return p.view(t.shape)


def poison(a: Audit, pattern: str, only: Optional[Callable[[str], bool]] = None) -> int:
    """Fills every SCRATCH cell with `pattern`; CONST, ZERO and CARRIED cells are left alone.  only(name): restrict to some
    entries (bisecting a failure: poison half the names, then one buffer, then one region).  Returns the cells poisoned."""
    n = 0
    with torch.no_grad():
        for e in a.entries.values():
            if only is not None and not only(e.name):
                continue
            m = e.scratch_mask()
            if bool(m.all()):
                e.owner.copy_(pattern_like(e.owner, pattern))
            else:
                e.owner.copy_(torch.where(m, pattern_like(e.owner, pattern), e.owner))
            n += int(m.sum())
    return n


# ---------------------------------------------------------------------------------------------------------------------------
# snapshot / verify
# ---------------------------------------------------------------------------------------------------------------------------
def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(_INT_VIEW[t.dtype])


def snapshot(a: Audit) -> Dict[Tuple[str, str], torch.Tensor]:
    """Copies of the CONST regions (the ZERO regions need none: their value is known)."""
    return {(e.name, label): e.owner[idx].detach().clone() for e, idx, label in a.regions(CONST)}


def _first_bad(bad: torch.Tensor, values: torch.Tensor):
    i = tuple(int(v) for v in bad.nonzero()[0])
    return i, values[i].item()


def failures(a: Audit, snap) -> List[str]:
    out = []
    for e, idx, label in a.regions(ZERO):
        v = e.owner[idx]
        bad = _bits(v) != 0
        if bool(bad.any()):
            i, val = _first_bad(bad, v.contiguous())
            out.append(f"{e.name}: ZERO region ({label}) holds {val!r} (bits {_bits(v)[i].item():#x}) at index {i} of the region, "
                       f"{int(bad.sum())} non-zero cells")
    for e, idx, label in a.regions(CONST):
        v, was = e.owner[idx], snap[(e.name, label)]
        bad = _bits(v) != _bits(was)
        if bool(bad.any()):
            i, val = _first_bad(bad, v.contiguous())
            out.append(f"{e.name}: CONST region ({label}) changed at index {i}: {was.contiguous()[i].item()!r} -> {val!r}, "
                       f"{int(bad.sum())} cells")
    return out


def verify(a: Audit, snap) -> None:
    """CONST regions bitwise unchanged since `snap`, ZERO regions all-zero BITS (so -0.0 fails)."""
    bad = failures(a, snap)
    assert not bad, "resident state was damaged:\n  " + "\n  ".join(bad)


# ---------------------------------------------------------------------------------------------------------------------------
# DESIGN.md's table
# ---------------------------------------------------------------------------------------------------------------------------
BEGIN = "<!-- BEGIN state_audit table (tests/state_audit.py: design_table) -->"
END = "<!-- END state_audit table -->"
_CONTAINERS = (("engine.Workspace", WORKSPACE_RULES), ("engine.EncoderPlan buffer set", ENCODER_SET_RULES),
               ("video._StreamState", STREAM_RULES), ("video._BiState", BISTATE_RULES), ("train_loop.LoopBuffers (a / b)", LOOP_RULES))


def design_table() -> str:
    """The classification as DESIGN.md prints it: every CONST / ZERO rule by name, the SCRATCH names as one row per container."""
    lines = ["| container | buffers | class | region |", "|---|---|---|---|"]
    for title, rules in _CONTAINERS:
        groups: "OrderedDict[Tuple[str, str], List[str]]" = OrderedDict()
        for name, r in rules.items():
            groups.setdefault((r.doc_class, r.doc), []).append(name)
        for (cls, doc), names in groups.items():
            if cls != SCRATCH:
                lines.append(f"| {title} | {', '.join('`' + n + '`' for n in names)} | {cls} | {doc} |")
        rest = [n for n, r in rules.items() if r.doc_class == SCRATCH]
        lines.append(f"| {title} | {', '.join('`' + n + '`' for n in rest)} | SCRATCH | all of it; and every cell of the rows "
                     "above that no region claims |")
    return "\n".join(lines)
