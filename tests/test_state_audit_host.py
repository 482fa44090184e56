"""tests/state_audit.py on the host: the REAL containers (engine.Workspace, the encoders' buffer sets, video._StreamState /
_BiState on the host emulation library, train_loop.LoopBuffers in plain torch) are fully classified, with regions in bounds,
disjoint and views counted once; and a toy state with a toy forward shows that every kind of fault the audit exists for is
reported -- and that the unfaulted toy passes."""
import pytest
import torch

import emu_lib
import state_audit as sa


@pytest.fixture(scope="module")
def lib():
    return emu_lib.load()


def _check_regions(a: sa.Audit):
    """Every region in bounds and disjoint (Audit._classify raises otherwise; here the sum rule: the classes partition each
    storage), every storage once."""
    ptrs = [e.owner.untyped_storage().data_ptr() for e in a.entries.values()]
    assert len(set(ptrs)) == len(ptrs)
    for e in a.entries.values():
        assert e.owner.numel() * e.owner.element_size() == e.owner.untyped_storage().nbytes(), e.name
        claimed = torch.zeros(e.owner.shape, dtype=torch.int32)
        for _cls, idx, _label in e.regions:
            claimed[idx] += 1
        assert int(claimed.max()) <= 1, e.name
        assert int(claimed.sum()) + int(e.scratch_mask().sum()) == e.owner.numel(), e.name


@pytest.mark.parametrize("H,W,f16,alt", [(128, 256, False, False), (128, 256, True, False), (128, 256, False, True),
                                         (128, 256, True, True), (136, 216, False, False)])
def test_workspace_is_fully_classified(lib, H, W, f16, alt):
    """Every (f16, alt_corr) form of the workspace at the smallest shape, and the ragged shape once."""
    from prior_flow_amd.engine import Workspace
    ws = Workspace(lib, 1, H, W, "cpu", f16=f16, alt_corr=alt)
    a = sa.audit(("ws", ws))
    _check_regions(a)
    names = a.names()
    # views are not entries of their own: they are aliases of the storage's owner
    for view, owner in (("ws.net_a[0]", "ws.net0_ab"), ("ws.net_b[0]", "ws.net0_ab"), ("ws.x_a", "ws.x_ab"), ("ws.x_b", "ws.x_ab"),
                        ("ws.f.f1a", "ws.f_all"), ("ws.f.f2b", "ws.f_all"), ("ws.net_a_s[0]", "ws.net0_ab_s"), ("ws.x_b_s", "ws.x_ab_s")):
        assert view not in names and a.entry(view).name == owner
    assert "ws.net_a[1]" in names and "ws.pre[('a', '1')]" in names
    assert (("ws.pyr_a[3]" in names), ("ws.feat_b[2]" in names), ("ws.f_split" in names)) == (not alt, alt, not alt)
    rows = ws.B * ws.N
    const = {e.name for e, _, _ in a.regions(sa.CONST)}
    assert const == {"ws.g_a2b", "ws.g_a2b_8", "ws.g_b2a_8", "ws.g_a2b_8_il", "ws.g_b2a_8_il", "ws.coords0"}
    zero = {e.name: [] for e, _, _ in a.regions(sa.ZERO)}
    for e, idx, _ in a.regions(sa.ZERO):
        zero[e.name].append(int(e.owner[idx].numel()))
    # the comments of engine.Workspace, as cell counts: cat_b 256..271; cat_b_s's last chunk / 64 columns; cat_a_s past 272
    assert zero["ws.cat_b"] == [rows * 16]
    assert zero["ws.cat_b_s"] == [rows * (64 if f16 else 2 * 32)]
    assert zero["ws.cat_a_s"] == [rows * (48 if f16 else 2 * 16)]
    assert set(zero) == {"ws.cat_b", "ws.cat_b_s", "ws.cat_a_s"}       # 128 and 256 channels fill their last chunk
    # poisoning leaves exactly those alone
    snap = sa.snapshot(a)
    for pattern in sa.PATTERNS:
        sa.poison(a, pattern)
        sa.verify(a, snap)
    assert float(ws.cat_b[:, :256].abs().min()) > 9e29 and not ws.cat_b[:, 256:].any()
    assert bool((ws.net0_ab_s.float().abs() > 5e4).all())


def test_encoder_sets_streams_and_loop_buffers_are_fully_classified(lib):
    from prior_flow_amd._lib import PREC_BF16X3
    from prior_flow_amd.engine import EncoderPlan, split_twin
    from prior_flow_amd.modules import build_tree
    from prior_flow_amd.train_loop import LoopBuffers
    from prior_flow_amd.video import _BiState, _StreamState
    fnet, cnet, _, _ = build_tree(0.0)
    plans = (EncoderPlan(lib, cnet, PREC_BF16X3), EncoderPlan(lib, fnet, PREC_BF16X3))
    plans[0]._alloc(2, 128, 256)
    plans[0]._alloc_folded(2, 128, 256)
    plans[1]._alloc(4, 128, 256)
    plans[1]._alloc(2, 136, 216)
    # the twins _run_folded allocates when it knows which kernel a level takes: as that code makes them
    fold = plans[0]._bufs_by_key[("fold", 2, 128, 256)]
    r1 = fold["x1"][0].shape[0]
    fold["xs1"], fold["y1"] = [split_twin(r1, 96, "cpu"), split_twin(r1, 96, "cpu")], split_twin(r1, 96, "cpu")
    states = [("stream", _StreamState(lib, 1, 128, 256, "cpu", False, False)),
              ("stream_f16_alt", _StreamState(lib, 1, 128, 256, "cpu", True, True)),
              ("bi_twins", _BiState(lib, 1, 128, 256, "cpu", False, False, True)),
              ("bi_rows", _BiState(lib, 1, 128, 256, "cpu", True, False, False)),
              ("loop", LoopBuffers(1, 17, 27, 2, "cpu"))]
    with pytest.raises(sa.AuditError, match="clean point only"):
        sa.audit(states[-1], clean=False)
    for clean in (True, False):
        a = sa.audit(("cnet", plans[0]), ("fnet", plans[1]), *(states if clean else states[:-1]), clean=clean)
        _check_regions(a)
        names = a.names()
        assert "cnet['fold', 2, 128, 256].x1[1]" in names and "fnet[4, 128, 256].act0[3]" in names and "fnet[2, 136, 216].part" in names
        # a stream's views into its own workspace count once, under the workspace
        assert "stream.img_new" not in names and a.entry("stream.img_new").name == "stream.ws.img_f"
        assert a.entry("stream.f4").name == "stream.ws.f_all" and a.entry("stream.s4").name == "stream.ws.f_split"
        assert a.entry("bi_twins.img_slot").name == "bi_twins.ws.img_c"
        assert "bi_twins.cn_x_s[1]" in names and "bi_rows.cn_x[0]" in names
        if clean:
            assert "loop.a.F[3]" in names and "loop.b.flow2" in names
            z = {e.name: e.owner[idx] for e, idx, _ in a.regions(sa.ZERO)}
            assert tuple(z["loop.a.d_delta"].shape) == (2, 17 * 27, 2) and tuple(z["loop.a.d_out"].shape) == (2, 17 * 27, 4)
            assert tuple(z["loop.b.d_out"].shape) == (2, 17 * 27, 2)
        carried = {e.name for e, _, _ in a.regions(sa.CARRIED)}
        if clean:
            assert not carried
        else:       # a running stream keeps its cached frame and flow
            assert {"stream.flow_low", "stream.ws.img_c", "stream.ws.f_all", "bi_twins.cn_net[0]"} <= carried
            assert "stream.ws.net0_ab" not in carried
            before = states[0][1].flow_low.clone()
            sa.poison(a, "nan")
            assert torch.equal(states[0][1].flow_low, before) and bool(torch.isnan(states[0][1].ws.net0_ab).all())
            assert bool(torch.isnan(states[0][1].ws.f_all.view(2, 2, -1, 256)[:, 1]).all())
            assert not states[0][1].ws.f_all.view(2, 2, -1, 256)[:, 0].any()


# ---- planted faults on a toy ------------------------------------------------------------------------------------------------
class Toy:
    """table: CONST.  buf [4, 8]: columns 6, 7 ZERO (padding), the rest SCRATCH.  tmp [4, 6]: SCRATCH."""

    def __init__(self):
        self.table = torch.arange(8, dtype=torch.float32)
        self.buf = torch.zeros(4, 8)
        self.tmp = torch.zeros(4, 6)
        self.half = torch.zeros(4, 2, 2, 32, dtype=torch.bfloat16)       # a split twin of 40 channels


TOY_RULES = {"table": sa.R_CONST("toy"), "buf": sa.R_COLS(6, "toy"), "tmp": sa.R_SCRATCH(),
             "half": sa.Rule(lambda holder, name, t: sa.operand_zero_regions(t, 40, 40), sa.ZERO, "toy")}


def relu(v):
    """The device ReLU, fmaxf(v, 0): a NaN operand gives 0 (torch.clamp_min would propagate it)."""
    return torch.fmax(v, torch.zeros_like(v))


def toy_forward(s: Toy, x: torch.Tensor, fault=None) -> torch.Tensor:
    """out[r] = sum_c (2 x[r, c] + table[c]) through the resident buffers."""
    extra = 0.0
    if fault == "stale_read":
        extra = s.tmp[:, 4].clone()                 # read before the write below
    if fault == "stale_read_behind_relu":
        extra = relu(s.tmp[:, 4:6]).sum(1)
    s.tmp.copy_(2 * x)
    v = s.tmp + s.table[:6]
    if fault == "write_into_zero":                  # one column too far
        s.buf[:, :7] = torch.cat([v, torch.ones(4, 1)], 1)
    else:
        s.buf[:, :6] = v
    if fault == "negative_zero":
        s.buf[:, 7] = -0.0
        s.half[:, 1, 1, 8:] = -0.0
    if fault == "const_edit":
        s.table[7] += 1                             # (an entry the output does not use)
    s.half[:, 0, 0, :] = 1
    s.half[:, 1, 0, :8] = 1
    return s.buf[:, :6].sum(1) + extra


def _toy_run(fault, pattern):
    """-> (the poisoned call's output equals the fresh one's bit for bit, verify's failures)."""
    x = torch.arange(24, dtype=torch.float32).view(4, 6) / 7
    want = toy_forward(Toy(), x, fault)
    s = Toy()
    a = sa.Audit().add("toy", s, rules=TOY_RULES)
    snap = sa.snapshot(a)
    toy_forward(s, x + 1, fault)            # a first call on other inputs: the state a real caller leaves behind
    bad = sa.failures(a, snap)
    snap = sa.snapshot(a) if fault == "const_edit" else snap
    sa.poison(a, pattern)
    got = toy_forward(s, x, fault)
    return torch.equal(got.view(torch.int32), want.view(torch.int32)), bad + sa.failures(a, snap)


@pytest.mark.parametrize("pattern", sa.PATTERNS)
def test_unfaulted_toy_passes(pattern):
    same, bad = _toy_run(None, pattern)
    assert same and not bad, bad


@pytest.mark.parametrize("pattern", sa.PATTERNS)
def test_stale_read_is_reported(pattern):
    same, bad = _toy_run("stale_read", pattern)
    assert not same and not bad


def test_stale_read_behind_a_relu_needs_the_big_pattern():
    """fmaxf(NaN, 0) = 0 is what the cell held at allocation: the NaN pattern alone cannot see this read; +-1e30 can."""
    same_nan, _ = _toy_run("stale_read_behind_relu", "nan")
    same_big, _ = _toy_run("stale_read_behind_relu", "big")
    assert same_nan, "the NaN pattern caught a read behind a ReLU: the toy no longer models fmaxf"
    assert not same_big


@pytest.mark.parametrize("fault,what", [("write_into_zero", "toy.buf: ZERO region (columns 6..7) holds 1.0"),
                                        ("negative_zero", "toy.buf: ZERO region (columns 6..7) holds -0.0"),
                                        ("const_edit", "toy.table: CONST region (all) changed at index (7,): 7.0 -> 8.0")])
def test_damage_to_zero_and_const_regions_is_reported(fault, what):
    same, bad = _toy_run(fault, "nan")
    assert same                                 # the output does not show it: only verify does
    assert any(what in b for b in bad), bad
    if fault == "negative_zero":                # integer views: -0.0 == 0.0 as floats; the twin's pad lanes are checked alike
        assert any("toy.half: ZERO region (pad lanes 8..31 of chunk 1" in b and "bits -0x8000" in b for b in bad), bad
        assert "index (0, 1)" in [b for b in bad if "toy.buf" in b][0]
    with pytest.raises(AssertionError, match="resident state was damaged"):
        sa.verify(*_damaged(fault))


def _damaged(fault):
    s = Toy()
    a = sa.Audit().add("toy", s, rules=TOY_RULES)
    snap = sa.snapshot(a)
    toy_forward(s, torch.zeros(4, 6), fault)
    return a, snap


def test_unclassified_attribute_is_an_error():
    s = Toy()
    s.extra = [torch.zeros(3)]
    with pytest.raises(sa.AuditError, match=r"toy\.extra\[0\].*is not classified"):
        sa.Audit().add("toy", s, rules=TOY_RULES)
    from prior_flow_amd.train_loop import LoopBuffers
    loop = LoopBuffers(1, 16, 32, 1, "cpu")
    loop.a["d_new"] = torch.zeros(4)
    with pytest.raises(sa.AuditError, match=r"loop\.a\.d_new \(a LoopBuffers's `d_new`\) is not classified"):
        sa.audit(("loop", loop))


def test_regions_out_of_bounds_or_overlapping_are_errors():
    s = Toy()
    with pytest.raises(sa.AuditError, match="out of bounds"):
        sa.Audit().add("toy", s, rules=dict(TOY_RULES, buf=sa.R_COLS(8, "toy")))
    two = sa.Rule(lambda h, n, t: [(sa.ZERO, (slice(None), slice(6, 8)), "a"), (sa.CONST, (slice(0, 1), slice(7, 8)), "b")], sa.ZERO, "")
    with pytest.raises(sa.AuditError, match="overlaps"):
        sa.Audit().add("toy", s, rules=dict(TOY_RULES, buf=two))
    with pytest.raises(sa.AuditError, match=r"expected \[rows, 9, 2, 32\]"):
        sa.operand_zero_regions(torch.zeros(4, 8, 2, 32, dtype=torch.bfloat16), 272, 256)


def test_poison_patterns_are_the_documented_bits():
    for dt, nan_bits in ((torch.float32, 0x7fc00000), (torch.float16, 0x7e00), (torch.bfloat16, 0x7fc0), (torch.int32, -1)):
        p = sa.pattern_like(torch.zeros(5, dtype=dt), "nan")
        assert p.dtype == dt and p.view(sa._INT_VIEW[dt]).tolist() == [nan_bits] * 5
    assert bool(torch.isnan(sa.pattern_like(torch.zeros(3, dtype=torch.float64), "nan")).all())
    assert sa.pattern_like(torch.zeros(4), "big").tolist() == [torch.tensor(1e30).item(), -torch.tensor(1e30).item()] * 2
    assert sa.pattern_like(torch.zeros(2, dtype=torch.float16), "big").tolist() == [60000.0, -60000.0]
    assert sa.pattern_like(torch.zeros(2, dtype=torch.float64), "big").tolist() == [1e300, -1e300]
    assert sa.pattern_like(torch.zeros(2, dtype=torch.int32), "big").tolist() == [0x7fffffff] * 2
    assert bool(torch.isfinite(sa.pattern_like(torch.zeros(2, dtype=torch.bfloat16), "big").float()).all())
