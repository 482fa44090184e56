"""The launch cases of tests/alt_corr_launches.py without a GPU: the case table is the one the suite promises, the bound's count
is the one written next to the reference, the corner restatement reproduces the float64 reference, the stretch sweep meets its
own conditions (rounding immunity, a unit on LF_CAP and one just above it), deliberate mistakes fail the bound, and the host
emulation of pf_lookup_feat_elem passes every case the GPU runs against the same reference and bound.  Path counts do not exist
in the elem form: here the prediction is checked against its own conditions only."""
import math
import os

import pytest
import torch

import alt_corr_launches as al
import alt_corr_ref as ref
import elem_launches as el

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def emu():
    import emu_lib
    return emu_lib.load()


@pytest.fixture(scope="module")
def table():
    t = el.Table()
    yield t
    print("\nhost emulation, worst |err| / bound\n" + t.render())


def test_case_table_is_the_promised_one():
    assert list(al.MAPS.values()) == [(1, 16, 16), (3, 17, 27), (2, 18, 21), (1, 16, 34), (1, 20, 45)]
    assert al.CHANNELS == (4, 36, 128, 256, 260, 512) and al.FAMILIES == ("zero", "nasty", "large", "outside")
    assert {(C, f) for C, m, f in al.CASES if m == "17x27"} == {(C, f) for C in al.CHANNELS for f in al.FAMILIES}
    assert {(m, f) for C, m, f in al.CASES if C == 256} == {(m, f) for m in al.MAPS for f in al.FAMILIES}
    assert len(al.CASES) == len(set(al.CASES)) == 24 + 16
    assert al.STRETCH == ((1, 1), (2, 2), (2, 3)) and al.STRETCH_MAP == (1, 32, 64) and len(al.STRETCH_CASES) == 3
    # partial tiles: dead waves per last-column tile, a dead tile row
    assert [(-w) % ref.LF_TX for _, _, w in al.MAPS.values()] == [0, 1, 3, 2, 3]
    assert [h % ref.LF_TY for _, h, _ in al.MAPS.values()] == [0, 1, 0, 0, 0]
    # the constants restated from the kernel
    text = open(os.path.join(ROOT, "prior-flow_amd", "csrc", "pf_lookup.hip")).read()
    assert "constexpr int LF_TY = 2, LF_TX = 4, LF_WAVES = LF_TY * LF_TX;" in text and "constexpr int LF_CAP = 192;" in text
    assert "constexpr int LF_CH = 32;" in text and "const bool tiled = nwin <= LF_CAP;" in text
    assert (ref.LF_TY, ref.LF_TX, ref.LF_CAP) == (2, 4, 192)
    # one channel count per branch: lanes without channels, a ragged last chunk, a second channel group partly / fully set
    assert [C % 32 for C in al.CHANNELS] == [4, 4, 0, 0, 4, 0] and [C > 256 for C in al.CHANNELS] == [False] * 4 + [True] * 2


def test_bound_counts_the_terms_of_the_code():
    assert ref.U == 2.0 ** -24
    assert [ref.k_terms(C) for C in al.CHANNELS] == [C + 15 + 1 + 4 for C in al.CHANNELS]
    mag = torch.tensor([2.0], dtype=torch.float64)
    assert float(ref.bound(256, mag)) == (256 + 20 + 1) * 2.0 ** -24 * 2.0


def test_outside_family_leaves_the_own_view_without_a_corner():
    """nwin == 0 in every own-view unit (the tile path with nu == 0), at every level."""
    for name in ("17x27", "16x16"):
        c = al.make_case(4, name, "outside")
        corn = ref.corners(c["coords"], c["g"])
        nwin, counts = ref.units(corn, c["B"], c["h"], c["w"])
        assert bool((nwin[:, :, 0] == 0).all()) and sum(counts) == al.n_units(c["B"], c["h"], c["w"])
        assert all(bool((lv["own"][1] == 0).all()) for lv in corn)
        # the cross view reads the level-0 grid at level-i coordinates: off the grid at levels 0 and 1 (the sample returns (0, 0),
        # one corner, element 0), on it again at levels 2 and 3 (y / 4 and y / 8 are rows of the map)
        assert bool((nwin[:, :2, 1] == 1).all()) and bool((nwin[:, 2:, 1] >= 1).all()) and int(nwin[:, 2:, 1].max()) > 1


def test_both_paths_are_predicted_on_the_ragged_map():
    """The decision does not depend on C: the families of (3, 17, 27) reach both paths, so every channel count does."""
    tot = [0, 0]
    for f in al.FAMILIES:
        c = al.make_case(4, "17x27", f)
        _, counts = ref.units(ref.corners(c["coords"], c["g"]), c["B"], c["h"], c["w"])
        print(f, counts)
        tot = [tot[0] + counts[0], tot[1] + counts[1]]
    assert tot[0] > 100 and tot[1] > 100, tot


@pytest.mark.parametrize("key", [(36, "17x27", "nasty"), (256, "32x64", "stretch2x3")], ids=str)
def test_corner_restatement_reproduces_the_reference(key):
    """sum_j w_j V[e_j] over the corners of alt_corr_ref.corners is the value of alt_corr_ref.lookup_feat: the indices and weights
    the path prediction is built from are those of the reference the values are checked against."""
    c = al.make_case(*key)
    B, C, h, w = c["B"], c["C"], c["h"], c["w"]
    N = h * w
    want = ref.lookup_feat(c["coords"], c["f1a"], c["f2a"], c["f1b"], c["f2b"], c["g"])
    corn = ref.corners(c["coords"], c["g"])
    for v, (key_, f1, f2) in enumerate((("own", c["f1a"], c["f2a"]), ("raw", c["f1b"], c["f2b"]))):
        a = f1.double().permute(0, 2, 3, 1).reshape(B, N, C)
        for i, lv in enumerate(ref.pool_levels(f2.double())):
            vol = torch.matmul(a, lv.reshape(B, C, -1)).reshape(B * N, -1) / math.sqrt(C)
            idx, wgt = corn[i][key_]
            vals = torch.gather(vol, 1, idx.clamp_min(0).reshape(B * N, -1)).reshape(idx.shape)
            got = (vals * wgt.double() * (idx >= 0)).sum(-1)
            assert float((got - want[v][:, 81 * i:81 * (i + 1)]).abs().max()) < 1e-12, (key_, i)


def test_stretch_sweep_meets_its_own_conditions(capsys):
    sweep = al.stretch_sweep()                                      # asserts immunity or decidedness, the cap and cap + 1 row units
    with capsys.disabled():
        for c, p in sweep:
            print(f"\n{c['family']}: predicted [tiled, pixel] = {p['counts']}, {p['masked']} of {p['nwin'].numel()} units masked "
                  f"(window rows {p['masked_nwin']}), exact = {p['exact']}")
    assert [p["counts"] for _, p in sweep] == [[1850, 198], [1872, 176], [1869, 179]]
    # the decision is not trivially one-sided, and the cap itself is met from both sides in the sweep
    assert all(min(p["counts"]) > 100 for _, p in sweep)


def test_a_position_next_to_an_integer_is_not_immune():
    p = torch.tensor([0.0, 1 / 16, 15 / 16, 7.5, 3.0, 1 / 32, 2 + 31 / 32, -0.5, -1 / 32])
    assert al.immune(p).tolist() == [True, True, True, True, False, False, False, True, False]
    # the real rotation grid is not immune: its path counts are not asserted
    c = al.make_case(4, "16x16", "nasty")
    assert not al.pin(c)["exact"]


@pytest.mark.parametrize("mistake", ["dropped_chunk", "no_scale", "wrong_corner", "level_off"])
def test_structural_mistakes_fail_the_bound(mistake):
    """What the suite is for: errors of order 1e-2 of the magnitude, hundreds of times the bound."""
    c = al.make_case(36, "17x27", "zero")
    good = al.reference(c)
    bad = dict(c)
    if mistake == "dropped_chunk":                                  # the ragged last chunk of the tile path is never added
        bad["f2a"], bad["f2b"] = c["f2a"].clone(), c["f2b"].clone()
        bad["f2a"][:, 32:] = 0
        bad["f2b"][:, 32:] = 0
    elif mistake == "no_scale":
        bad["f1a"], bad["f1b"] = c["f1a"] * math.sqrt(36.0), c["f1b"] * math.sqrt(36.0)
    elif mistake == "wrong_corner":
        bad["coords"] = c["coords"] + torch.tensor([1.0, 0.0]).view(1, 2, 1, 1)
    else:                                                           # stale rows: the window of another level's map
        bad["f2a"], bad["f2b"] = torch.roll(c["f2a"], 1, 2), torch.roll(c["f2b"], 1, 2)
    wrong = al.reference(bad)
    for what in ("own", "raw"):
        r = el.ratio(wrong[what][0], *good[what])
        assert r > 100, (mistake, what, r)


@pytest.mark.parametrize("key", al.CASES + al.STRETCH_CASES, ids=lambda k: f"C{k[0]}-{k[1]}-{k[2]}")
def test_emulation_passes(emu, table, key):
    """Every case of the GPU test through pf_lookup_feat_elem, with everything the GPU test asks of a launch but the path
    counts: values, padding, NaN prefill, the second launch, the B = 1 launch of every image."""
    c = al.make_case(*key)
    fails, _ = al.run_case(emu, c, CPU, table, counts=False)
    assert not fails, "\n".join(fails)
