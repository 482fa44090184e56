"""pf_dccl_lookup_feat (pf_lookup_feat_kernel) on the MI355X at ragged maps, every channel layout and both paths, against the
float64 restatement under the derived bound of tests/alt_corr_ref.py; the path decision pinned unit by unit on the stretch
sweep; the alternate_corr forward at the two ragged golden sizes.  Cases: tests/alt_corr_launches.py, which the host emulation
runs as well (tests/test_alt_corr_launch_reference.py).  Run with ``-m gpu``.

MI355X, worst |err| / bound, bound = (C + 21) 2^-24 sum |term| (the worse of own and raw, all rows, all 324 columns; the table is
printed again at the end of this module):

    map (B, h, w)    C     zero    nasty   large   outside
    (3, 17, 27)      4     0.133   0.149   0.131   0.070
    (3, 17, 27)      36    0.083   0.047   0.036   0.052
    (3, 17, 27)      128   0.023   0.014   0.011   0.018
    (3, 17, 27)      256   0.016   0.007   0.011   0.011
    (3, 17, 27)      260   0.016   0.009   0.007   0.012
    (3, 17, 27)      512   0.008   0.005   0.003   0.004
    (1, 16, 16)      256   0.010   0.009   0.007   0.010
    (2, 18, 21)      256   0.012   0.009   0.007   0.008
    (1, 16, 34)      256   0.014   0.006   0.011   0.006
    (1, 20, 45)      256   0.015   0.006   0.007   0.009
    (1, 32, 64)      256   stretch 1x1 0.007, 2x2 0.007, 2x3 0.007

The ratios fall with C as 1 / sqrt(C) does: the bound is the worst case of C terms of one sign, the data have random signs.

Stretch sweep on (1, 32, 64), C = 256, [tile path, pixel path] units of 2048, predicted from alt_corr_ref.corners and measured:

    (sx, sy)   predicted      measured       masked units (window rows)
    (1, 1)     [1850, 198]    [1850, 198]    224 (0 .. 112)
    (2, 2)     [1872, 176]    [1872, 176]    72  (4 .. 112)      76 units hold exactly LF_CAP = 192 rows
    (2, 3)     [1869, 179]    [1869, 179]    120 (4 .. 54)       43 units hold 193 .. 224 rows

Units per channel count over all cases, [tile path, pixel path]: 4: [5219, 829], 36: [5219, 829], 128: [5209, 839],
256: [19676, 3140], 260: [5221, 827], 512: [5220, 828].
"""
import argparse

import pytest
import torch

import alt_corr_launches as al
import elem_launches as el
import golden_cases as gc
import priorflow_oracle as po

pytestmark = pytest.mark.gpu
EPE_BAR = 1e-3                       # tests/test_hip_forward.py, tests/test_hip_alt_corr.py
SIZES = [(136, 216), (160, 360)]     # 1/8 maps of 17 x 27 and 20 x 45: golden `forward_odd`


@pytest.fixture(scope="module")
def lib():
    from prior_flow_amd import _lib
    return _lib.load()               # raises if the HIP library was not built: no fallback


@pytest.fixture(scope="module")
def table():
    t = el.Table()
    yield t
    print("\nMI355X, worst |err| / bound\n" + t.render())


@pytest.fixture(scope="module")
def ledger():
    """[tile path, pixel path] units summed per channel count over the cases of this module that ran."""
    return {}


def _book(ledger, C, cnt):
    have = ledger.setdefault(C, [0, 0])
    ledger[C] = [have[0] + cnt[0], have[1] + cnt[1]]


# ---- launches -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", al.CASES, ids=lambda k: f"C{k[0]}-{k[1]}-{k[2]}")
def test_launch_matches_float64(lib, table, ledger, key):
    c = al.make_case(*key)
    fails, cnt = al.run_case(lib, c, torch.device("cuda:0"), table, counts=True)
    print(f"{key}: [tile, pixel] units {cnt}")
    assert not fails, "\n".join(fails)
    _book(ledger, c["C"], cnt)
    if c["family"] == "outside":     # no own-view corner anywhere: half of the units at least take the tile path with nu == 0
        assert cnt[0] >= al.n_units(c["B"], c["h"], c["w"]) // 2


@pytest.fixture(scope="module")
def sweep():
    return al.stretch_sweep()        # the builder's own asserts: immune or decided everywhere, a unit on the cap, one just above


@pytest.mark.parametrize("i", range(len(al.STRETCH)), ids=[k[2] for k in al.STRETCH_CASES])
def test_stretch_sweep_takes_the_predicted_paths(lib, table, ledger, sweep, i):
    """The units of a launch that take each path are the ones whose window the restatement puts at or under, or over, LF_CAP:
    exactly, because no floor of the family can round the other way (alt_corr_launches.pin).  The prediction is masked where the
    constant grid meets the map border; every masked unit is decided by a bracket of its window, so all three launches compare."""
    c, p = sweep[i]
    fails, cnt = al.run_case(lib, c, torch.device("cuda:0"), table, counts=True)
    print(f"{c['family']}: predicted {p['counts']}, measured {cnt}; {p['masked']} units masked, window rows {p['masked_nwin']}")
    assert not fails, "\n".join(fails)
    assert p["exact"]
    assert cnt == p["counts"], (c["family"], cnt, p["counts"])
    _book(ledger, c["C"], cnt)


def test_both_paths_taken_at_every_channel_count(lib, ledger):
    """Summed over the cases above; a channel count whose cases did not run in this session (a -k selection) launches its four
    families on (3, 17, 27) here, counts only."""
    dev = torch.device("cuda:0")
    for C in al.CHANNELS:
        if C not in ledger:
            for f in al.FAMILIES:
                _, _, cnt = al.launch(lib, al.make_case(C, "17x27", f), dev, counts=True)
                _book(ledger, C, cnt)
    print("units per channel count [tile path, pixel path]:", ledger)
    assert sorted(ledger) == sorted(al.CHANNELS)
    for C, (tiled, pixel) in ledger.items():
        assert tiled > 0 and pixel > 0, (C, tiled, pixel)


# ---- forward --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def params():
    from prior_flow_amd.modules import state_dict_shapes
    return gc.det_state_dict(state_dict_shapes())


def make_model(params, **args):
    from prior_flow_amd.prior_raft import PriOr_RAFT
    m = PriOr_RAFT(argparse.Namespace(**dict(dict(mixed_precision=False, dropout=0.0), **args)))
    m.load_state_dict(params, strict=True)
    return m.cuda().eval()


def epe(a, b):
    b = b if isinstance(b, torch.Tensor) else torch.from_numpy(b)
    e = po.epe(a.detach().cpu().float(), b.detach().cpu().float())
    return float(e.mean()), float(e.max())


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_forward_alternate_at_ragged_maps(params, size):
    """1/8 maps of 17 x 27 and 20 x 45: partial 2 x 4 tiles at every launch of every iteration.  test_mode returns branch A."""
    h, w = size
    i1, i2 = gc.synthetic_pair(1, h, w, seed=31)
    i1, i2 = i1.cuda(), i2.cuda()
    alt, default = make_model(params, alternate_corr=True), make_model(params)
    with torch.no_grad():
        alt.use_graph = False
        eager = alt(i1, i2, iters=3, test_mode=True)
        alt.use_graph = True
        g1 = alt(i1, i2, iters=3, test_mode=True)
        g2 = alt(i1, i2, iters=3, test_mode=True)
        want = default(i1, i2, iters=3, test_mode=True)
    assert eager.shape == (1, 2, h, w) and all(ws.alt_corr and ws.pyr_a is None for ws in alt._ws.values())
    m_gold, x_gold = epe(eager, gc.load("forward_odd")[f"a_{h}x{w}"])
    m_def, x_def = epe(eager, want)
    print(f"{h}x{w}: mean EPE {m_gold:.3e} (max {x_gold:.3e}) against the golden, {m_def:.3e} (max {x_def:.3e}) against the default mode")
    assert m_gold < EPE_BAR, (size, m_gold, x_gold)
    assert m_def < EPE_BAR, (size, m_def, x_def)
    assert not torch.equal(eager, want)                  # a different arithmetic, not the default path under another name
    assert torch.equal(g1, g2), "graph replay must be deterministic"
    assert torch.equal(g1, eager), "graph replay differs from eager launches"


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_forward_mixed_precision_with_alternate_at_ragged_maps(params, size):
    h, w = size
    i1, i2 = gc.synthetic_pair(1, h, w, seed=31)
    with torch.no_grad():
        mixed = make_model(params, mixed_precision=True)(i1.cuda(), i2.cuda(), iters=3, test_mode=True)
        both = make_model(params, mixed_precision=True, alternate_corr=True)(i1.cuda(), i2.cuda(), iters=3, test_mode=True)
    assert bool(torch.isfinite(both).all())
    mean, mx = epe(both, mixed)
    print(f"{h}x{w} mixed_precision + alternate_corr vs mixed_precision: mean EPE {mean:.3e} max {mx:.3e}")
    assert mean < EPE_BAR, (size, mean, mx)
