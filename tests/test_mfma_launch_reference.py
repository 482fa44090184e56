"""The float64 references and bounds of tests/mfma_launches.py, checked without a GPU: against the CPU oracle and torch's float64
conv2d, against torch emulations of the device-only kernels' arithmetic (and the host emulation of the per-element entry points)
through the same cases the GPU test runs, and against deliberate mistakes, each of which must fail a bound at the smallest case of
its family.  The case table's own claims (which launcher path a case takes, that every selectable path is taken) are asserted here
as host logic."""
import os
import time

import pytest
import torch

import mfma_launches as ml
import priorflow_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "prior-flow_amd", "csrc")
CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def emu():
    import emu_lib
    return emu_lib.load()


@pytest.fixture(scope="module")
def table():
    t = ml.Table()
    yield t
    print("\ntorch / host emulation, worst |err| / bound\n" + t.render())


# ------------------------------------------------------------------------------------------------------------------------
# the case table
# ------------------------------------------------------------------------------------------------------------------------
def test_corr_select_restates_the_launcher():
    """The lines of corr_launch that corr_select mirrors are still there: a change of the dispatch must be noticed here."""
    text = open(os.path.join(CSRC, "pf_corr_mfma.hip")).read()
    for line in ("if (B <= 0 || H8 <= 0 || W8 <= 0 || C <= 0 || (C % KC) != 0) return PF_ERR_BAD_SHAPE;",
                 "if ((H8 >> 3) < 2 || (W8 >> 3) < 2) return PF_ERR_BAD_SHAPE;",
                 "a.scale_mul = (m == 0.5f && a.inv_scale * a.inv_scale == (float)C) ? 1.f / a.inv_scale : 0.f;",
                 "const bool fused = (W8 % 32) == 0 && (H8 % 8) == 0 && (a.N % BM) == 0;",
                 "const bool rs_on = !(rs_env && rs_env[0] == '0');",
                 "if (split && C == 32 * RING_NK && (W8 % 64) == 0 && rs_on) {",
                 "const int nch = (W8 % 128) == 0 ? 2 : 1;",
                 "const int RB = (H8 % 16) == 0 ? 16 : 8;",
                 "constexpr int BM = 128;", "constexpr int BN = 256;", "constexpr int KC = 32;", "constexpr int RING_NK = 8;"):
        assert line in text, line
    assert [ml.scale_is_exact(C) for C in (32, 64, 96, 256)] == [False, True, False, True]


def test_corr_cases_take_the_paths_they_are_for():
    sel = lambda n: ml.corr_select(*(ml.CORR_CASES[n][k] for k in "BHWC"), ml.CORR_CASES[n]["prec"] == ml.BF16X3, ml.CORR_CASES[n]["rs_on"])  # noqa: E731
    for shape in ("3x17x27", "1x16x24", "1x24x40"):
        for C in ((256, 32, 96, 64) if shape == "3x17x27" else (256,)):
            for p in ("fp32", "bf16x3"):
                assert sel(f"{shape}_c{C}_{p}") == ("generic", 0, 0, p, "mul" if C in (64, 256) else "div")
    for shape, C in (("2x16x32", 256), ("1x24x96", 256), ("2x16x32", 96)):
        for p in ("fp32", "bf16x3"):
            assert sel(f"{shape}_c{C}_{p}") == ("tile", 0, 0, p, "mul" if C == 256 else "div")
    assert sel("1x16x64_c256_bf16x3_rs0") == ("tile", 0, 0, "bf16x3", "mul")
    assert sel("1x16x64_c64_bf16x3") == ("tile", 0, 0, "bf16x3", "mul")           # W8 % 64 == 0 but C != 256
    assert sel("1x16x64_c256_bf16x3") == ("role-split", 16, 1, "bf16x3", "mul")
    assert sel("2x24x64_c256_bf16x3") == ("role-split", 8, 1, "bf16x3", "mul")
    assert sel("1x16x128_c256_bf16x3") == ("role-split", 16, 2, "bf16x3", "mul")
    assert sel("2x24x128_c256_bf16x3") == ("role-split", 8, 2, "bf16x3", "mul")
    assert sel("1x16x192_c256_bf16x3") == ("role-split", 16, 1, "bf16x3", "mul")
    # N = 459: ragged 128-row and 256-column tails; the poolings of 17 x 27 and of 8 x 13 drop a row / a column
    assert 459 % 128 and 459 % 256 and [((17 >> i) % 2, (27 >> i) % 2) for i in range(3)] == [(1, 1), (0, 1), (0, 0)]
    assert ml.case_env("corr", "1x16x64_c256_bf16x3_rs0") == {"PRIORFLOW_CORR_RS": "0"}
    assert all(ml.case_env(f, s) == {} for f, s in ml.CASES if not s.endswith("_rs0"))


def test_every_selectable_corr_path_has_a_case():
    """(kernel path, RB, chunk count, precision, scale branch): whatever corr_launch can select, some case selects."""
    hit = {ml.corr_select(c["B"], c["H"], c["W"], c["C"], c["prec"] == ml.BF16X3, c["rs_on"]) for c in ml.CORR_CASES.values()}
    want = ml.selectable_corr_paths()
    assert len(want) == 12 and want <= hit, sorted(want - hit)


def test_enc_stem_shapes_reach_the_second_tile():
    text = open(os.path.join(CSRC, "pf_enc_stem.hip")).read()
    assert "const long cap = 2L * cus;" in text and "a.tiles_x = (a.W2 + 31) / 32; a.tiles_y = (a.H2 + 7) / 8;" in text
    assert ml.stem_tiles(1, 16, 64) == (1, 1, 1) and ml.stem_tiles(2, 18, 70) == (2, 2, 8) and ml.stem_tiles(2, 128, 256)[2] == 64
    Bn, H, W = ml.stem_walk_shape(512)
    assert (Bn, H, W) == (5, 250, 522) and ml.stem_tiles(Bn, H, W) == (16, 9, 720)
    assert (H // 2) % 8 and (W // 2) % 32 and 720 - 512 == 208
    for cus in (64, 104, 228, 256, 304):
        n = ml.stem_tiles(*ml.stem_walk_shape(2 * cus))[2]
        assert n > 2 * cus and n % (2 * cus)
    # the CPU emulation walks the ragged shape's 8 tiles on 3 workgroups (ml.EmuOps.cap): a ragged third trip
    assert ml.stem_shape("walk", 3) == (2, 18, 70) and 8 > 3 and 8 % 3


# ------------------------------------------------------------------------------------------------------------------------
# references against the oracle / torch float64
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["3x17x27_c96_fp32", "1x16x24_c256_fp32"])
def test_corr_reference_matches_the_oracle(name, capsys):
    c = ml.CORR_CASES[name]
    B, H, W, C = (c[k] for k in "BHWC")
    f1, f2 = ml.corr_inputs(c, "spread", CPU)
    ref = ml.ref_corr(c, f1, f2)
    nchw = lambda f, dt: f.to(dt).view(B, H, W, C).permute(0, 3, 1, 2)           # noqa: E731
    pyr64 = po.build_pyramid(po.corr_volume(nchw(f1, torch.float64), nchw(f2, torch.float64)))
    pyr32 = po.build_pyramid(po.corr_volume(nchw(f1, torch.float32), nchw(f2, torch.float32)))
    worst = []
    for i, (r, b) in enumerate(ref):
        # the oracle divides by an fp32 sqrt(C) whatever the dtype of its inputs: one fp32 rounding of the divisor, none where exact
        rel = ml.U if not ml.scale_is_exact(C) else 1e-14
        assert bool(((pyr64[i].reshape(r.shape) - r).abs() <= rel * r.abs() + 1e-14).all())
        worst.append(ml.ratio(pyr32[i].reshape(r.shape), r, b))                # the fp32 oracle is inside the bounds
    with capsys.disabled():
        print(f"\nfp32 oracle, worst |err| / bound [{name}]: " + ", ".join(f"level {i} {v:.3f}" for i, v in enumerate(worst)))
    assert all(v <= 1.0 for v in worst), worst


def test_enc_stem_reference_matches_torch_float64_conv2d():
    img, w, b = ml.stem_case((2, 18, 70), CPU)
    v, bnd = ml.ref_enc_stem(img, w, b)
    want = torch.nn.functional.conv2d(img.double(), w.double(), b.double(), stride=2, padding=3).permute(0, 2, 3, 1).reshape(-1, 64)
    assert float((v - want).abs().max()) < 1e-13
    got32 = torch.nn.functional.conv2d(img, w, b, stride=2, padding=3).permute(0, 2, 3, 1).reshape(-1, 64)
    assert ml.ratio(got32, v, bnd) <= 1.0


def test_feature_pyramid_reference_matches_avg_pool2d():
    B, H, W, C = 3, 17, 27, 100
    x = torch.rand(B * H * W, C, generator=torch.Generator().manual_seed(3)) * 2 - 1
    cur = x.double().view(B, H, W, C).permute(0, 3, 1, 2)
    for r, _ in ml.ref_feat(x, B, H, W, C):
        cur = torch.nn.functional.avg_pool2d(cur, 2, stride=2)
        assert float((cur.permute(0, 2, 3, 1).reshape(-1, C) - r).abs().max()) < 1e-15


# ------------------------------------------------------------------------------------------------------------------------
# the emulations pass every case
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,shape", ml.cases("cpu"), ids=lambda v: str(v))
def test_emulation_passes(emu, table, family, shape, monkeypatch, capsys):
    """corr and enc_stem on the torch emulations of ml.emu_corr / ml.emu_enc_stem, the splits and the feature pyramid on the host
    emulation of csrc/pf_elem.h; the margin is the table printed at the end."""
    for k, v in ml.case_env(family, shape).items():
        monkeypatch.setenv(k, v)
    t0 = time.time()
    fails = ml.run_case(ml.EmuOps(emu), family, shape, CPU, table)
    with capsys.disabled():
        print(f" [{time.time() - t0:.1f} s]", end="")
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------------------------------
# deliberate mistakes fail
# ------------------------------------------------------------------------------------------------------------------------
def _mutant_fails(family, shape, mut, cap=3):
    fails = ml.run_case(ml.EmuOps(None, mut=mut, cap=cap), family, shape, CPU, ml.Table())
    return [f for f in fails if "|err|/bound" in f or "not split_bf16" in f]


@pytest.mark.parametrize("mut,shape", [
    ("drop_hilo", "1x16x24_c256_bf16x3"),           # a dropped hi * lo pass
    ("one_pass", "1x16x24_c256_bf16x3"),            # a single bf16 pass
    ("drop_chunk", "3x17x27_c96_fp32"),             # the last 32-channel chunk missing
    ("drop_chunk", "3x17x27_c96_bf16x3"),
    ("transpose", "1x16x24_c256_fp32"),             # n1 and n2 transposed
    ("batch_f2", "3x17x27_c32_fp32"),               # batch 1 reading batch 0's f2
    ("tile_shift", "1x16x24_c256_fp32"),            # one 32-column target tile shifted by one column
    ("pool_offset", "1x16x24_c256_fp32"),           # a pooled level taken from pairs offset by one
    ("pool_last", "3x17x27_c32_fp32"),              # odd-size pooling that takes the last row / column in
])
def test_corr_mistake_fails_a_bound(mut, shape):
    assert not _mutant_fails("corr", shape, None), "the unmutated emulation must pass"
    bad = _mutant_fails("corr", shape, mut)
    assert bad, f"{mut} passed every bound at {shape}"
    if mut.startswith("pool"):
        assert all("level 0" not in f for f in bad)


@pytest.mark.parametrize("mut,cap", [("second_tile", 3), ("second_tile", 4), ("stats_last_row", 3)])
def test_enc_stem_mistake_fails_a_bound(mut, cap):
    """The second tile of a workgroup written to the first tile's rows; a statistics partial that misses a partial tile's last
    row.  The ragged shape (2, 18, 70): 8 tiles of which the lower and right ones are partial."""
    assert not _mutant_fails("enc_stem", "walk", None, cap)
    bad = _mutant_fails("enc_stem", "walk", mut, cap)
    assert bad, f"{mut} passed every bound"
    assert any(("stats" in f) == (mut == "stats_last_row") for f in bad)


def test_flow_stem_emulation_passes_and_a_dropped_tap_row_fails(table):
    """pf_flow_stem_kernel exists only as device code: its bf16x3 arithmetic in torch is inside the bound of the 7x7 2 -> 128 layer
    (K = 98) at every geometry, and without the tap row that reads input row 0 at the top border it is outside."""
    for name, (B, H, W) in ml.GEOMS.items():
        x, w, b = ml._layer_data(torch.Generator().manual_seed(H), 2, 128, 7, B * H * W, CPU)
        v, bnd = ml.conv_ref(x, w, b, ml.BF16X3, B, H, W, 1)
        r = ml.ratio(ml.emu_flow_stem(x, w, b, B, H, W), v.clamp_min(0), bnd)
        table.add("pf_flow_stem_kernel (torch)", name, r)
        assert r <= 1.0, (name, r)
        got = ml.emu_flow_stem(x, w, b, B, H, W, mut="top_tap")
        bad = (got.double() - v.clamp_min(0)).abs() > bnd
        assert bool(bad.any()) and not bool(bad.view(B, H, W, 128)[:, 1:].any()), name


def test_conf_stem_without_the_inner_relu_fails():
    name = "1x16x32"
    B, H, W = ml.GEOMS[name]
    x, w1, b1, w2, b2 = ml.conf_case(name, CPU)
    want, bnd = ml.ref_conf_stem(x, w1, b1, w2, b2, B, H, W)
    assert ml.ratio(ml.emu_conf_stem(x, w1, b1, w2, b2, B, H, W), want, bnd) <= 1.0
    assert not ml.ratio(ml.emu_conf_stem(x, w1, b1, w2, b2, B, H, W, mut="no_relu"), want, bnd) <= 1.0


def test_conv_reference_matches_torch_float64_conv2d():
    """conv_ref (through conv_launches.conv_fp64) at both strides and kernel sizes the direct family uses, and the dispatch it
    restates against the limits in the source."""
    for cin, cout, k, stride in ((2, 128, 7, 1), (8, 32, 3, 2), (3, 64, 7, 2), (96, 32, 3, 1)):
        B, H, W = 2, 9, 13
        x, w, b = ml._layer_data(torch.Generator().manual_seed(k), cin, cout, k, B * H * stride * W * stride, CPU)
        v, _ = ml.conv_ref(x, w, b, ml.F32, B, H, W, stride)
        nchw = x.double().view(B, H * stride, W * stride, cin).permute(0, 3, 1, 2)
        want = torch.nn.functional.conv2d(nchw, w.double(), b.double(), stride=stride, padding=k // 2)
        assert float((want.permute(0, 2, 3, 1).reshape(-1, cout) - v).abs().max()) < 1e-12
    text = open(os.path.join(CSRC, "pf_elem_kernels.hip")).read()
    for line in ("const size_t lds = ((size_t)d.KH * (31 * d.stride + d.KW) * (d.Cin | 1) + 4 + 3 * 16 * 64) * 4;",
                 "if (lds <= 60 * 1024 && (K + 1) / 2 <= 160 &&",
                 "d.KH * (31 * d.stride + d.KW) * d.Cin <= 16 * 256 && d.Cin <= 255) {",
                 "return a.KH == 7 && a.KW == 7 && a.Cin == 2 && a.stride == 1 && !a.nchw && a.Cout % 64 == 0 && a.Ho == a.H && a.Wo == a.W &&",
                 "for (int i = 0; i < n; ++i) mf = mf && m.p[i].Cout == 128"):
        assert line in text, line
    kernels = {ml.direct_select(cin, cout, k, k, s, nchw, cout + 16, 8) for _, cin, cout, k, s, nchw, _ in ml.DIRECT_LAYERS}
    assert kernels == {"pf_flow_stem_kernel", "pf_stem7x7c2_valu", "pf_small_conv_mfma", "pf_direct_conv_elem"}
    assert all(ml.direct_select(cin, cout, k, k, s, nchw, cout + 16, 8) == want for _, cin, cout, k, s, nchw, want in ml.DIRECT_LAYERS)
