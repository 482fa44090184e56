"""The float64 references and bounds of tests/elem_launches.py, checked without a GPU: against the CPU oracle / torch autograd,
against the host emulation of csrc/pf_elem.h (the fixture of test_emu_kernels.py) through the same cases the GPU test runs, and
against deliberate mistakes applied to the reference output, each of which must fail the bound of the kernel it belongs to."""
import os
import shutil
import subprocess

import pytest
import torch

import elem_launches as el
import priorflow_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
EMU_SO = os.path.join(EMU_DIR, "libpf_emu.so")
CSRC = os.path.join(ROOT, "prior-flow_amd", "csrc")
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


def failed(got, ref, bound):
    return not el.ratio(got, ref, bound) <= 1.0


# ------------------------------------------------------------------------------------------------------------------------
# the case table itself
# ------------------------------------------------------------------------------------------------------------------------
def test_rows_shape_reaches_the_second_grid_stride_trip():
    """kMaxBlocks of csrc/pf_elem_kernels.hip is restated in the helper: a change there must be noticed here."""
    text = open(os.path.join(CSRC, "pf_elem_kernels.hip")).read()
    assert "constexpr long kMaxBlocks = 256L * 64;" in text
    assert el.K_MAX_BLOCKS == 256 * 64
    B, H, W = el.SHAPES["rows"]
    assert B * H * W > 4 * 16384                                   # a wave of the row kernels walks a second row
    assert B * H * W == el.ROW_COUNTS["rows"] == el.BN_ROWS["rows"]
    assert el.ROW_COUNTS["rows"] * 64 > 256 * el.K_MAX_BLOCKS      # the narrowest row-matrix launch loops too
    assert (B - 4) * H * W <= 4 * el.K_MAX_BLOCKS                  # and it is the smallest such batch (multiple of 4)


def test_case_table_covers_the_kernel_matrix():
    """Every kernel of a family appears in the table at every shape of the family; the shapes are the issue's."""
    assert list(el.SHAPES.items()) == [("even", (2, 16, 32)), ("ragged", (3, 17, 27)), ("folded", (1, 16, 16)), ("rows", (260, 16, 16))]
    assert [v[1:] for v in el.STAT_SHAPES.values()][:3] == [(64, 128), (459, 128), (240, 7)] and el.STAT_SHAPES["full"][1] == el.STAT_SHAPES["full"][2]
    # the row counts 1 / 200 / 66 560 of every row-matrix kernel: GRU gates, the norm kernels (B * Np), frozen BatchNorm
    assert list(el.ROW_COUNTS.values()) == [1, 200, 66560]
    assert [el.STAT_SHAPES[k][0] * el.STAT_SHAPES[k][1] for k in ("one", "some", "rows")] == [1, 200, 66560]
    assert sorted(el.BN_ROWS.values()) == [1, 17, 200, 459, 66560]
    assert el.STAT_SHAPES["rows"][2] == 128 and all(nb <= Np or k == "empty" for k, (_, Np, nb) in el.STAT_SHAPES.items())
    assert el.widths_of("rows") == (64, 96, 128) and el.widths_of("rows_c64") == (64,)       # all widths at every row count
    assert 66560 * 64 > 256 * el.K_MAX_BLOCKS            # the narrowest of them loops in a 256-thread elementwise kernel
    assert set(el.cases("gpu")) == set(el.CASES) and {c for c in el.cases("cpu") if c not in el.CASES} == {("warp", "rows_c64")}
    kernels = {k: set(shapes) for _, shapes, ks in el.FAMILIES.values() for k in ks}
    want = {"dccl_lookup": el.SHAPES, "dccl_lookup_il": el.SHAPES, "dccl_combine": el.SHAPES, "dccl_combine_bwd": el.SHAPES,
            "dccl_lookup_bwd": el.SHAPES, "pyramid_bwd": el.SHAPES, "coords_add": el.SHAPES, "coords_add_to": el.SHAPES,
            "warp_gcorr": el.SHAPES, "warp_gcorr+grid": el.SHAPES, "warp_gcorr_bwd": el.SHAPES, "upsample_flow": el.SHAPES,
            "upsample_flow_bwd": el.SHAPES, "flow_head_out": el.SHAPES, "flo_rotate": el.SHAPES, "motion_prep": el.SHAPES,
            "gru_q_bwd": el.ROW_COUNTS, "gru_zr_bwd": el.ROW_COUNTS, "gru_dx_finish": el.ROW_COUNTS,
            "channel_stats": el.STAT_SHAPES, "norm_act": el.STAT_SHAPES, "norm_bwd": el.STAT_SHAPES,
            "bn_frozen_fwd": el.BN_ROWS, "bn_frozen_bwd": el.BN_ROWS,
            "seq_loss": el.LOSS_SHAPES, "seq_loss_batch": el.LOSS_SHAPES, "sum_squares": el.LOSS_SHAPES,
            "adamw_step": el.LOSS_SHAPES, "adamw_step_dev": el.LOSS_SHAPES}
    assert {k: set(v) for k, v in want.items()} == kernels
    assert len(el.CASES) == len(set(el.CASES)) == sum(len(s) for _, s, _ in el.FAMILIES.values())


# ------------------------------------------------------------------------------------------------------------------------
# 2. the emulation passes every case (and fills the table every kernel must appear in)
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,shape", el.cases("cpu"), ids=lambda v: str(v))
def test_emulation_passes(emu, table, family, shape):
    """All shapes, and every kernel of the family in the table at that shape (el.run_case).  The 66 560-row cases run as they are,
    except the warp family: its row here is `rows_c64`, the same rows with 64 instead of 256 channels (el.CPU_SIBLINGS); the GPU
    runs the full width."""
    fails = el.run_case(emu, family, shape, CPU, table)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------------------------------
# 1. the float64 references equal the oracle / float64 autograd;  4. the fp32 oracle stays inside the bounds
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["even", "ragged"])
def test_lookup_reference_matches_the_oracle(shape, capsys):
    B, H, W = el.SHAPES[shape]
    c = el.lookup_case(shape, CPU, "real")
    refs = el.ref_lookup(c)
    as_pyr = lambda lv, dt: [p.to(dt).view(-1, 1, H >> i, W >> i) for i, p in enumerate(lv)]      # noqa: E731
    worst = {}
    for dt in (torch.float64, torch.float32):
        # an identity g_back makes the oracle's cross view the raw lookup itself (the rotation back is the combine's, below)
        own, raw = po.dccl_lookup(c["coords"].to(dt), as_pyr(c["own"], dt), as_pyr(c["oth"], dt), c["grid"].to(dt),
                                  po.coords_grid(1, H, W)[0].to(dt))
        own = own.permute(0, 2, 3, 1).reshape(-1, el.CORR_CH)
        if dt == torch.float64:
            assert float((raw.permute(0, 2, 3, 1).reshape(-1, el.CORR_CH) - refs["raw"][0]).abs().max()) < 1e-7
            # the oracle's pixel -> [-1, 1] -> pixel round trip and fmod are rounded in float64 too: 1e-9 covers them, except
            # where the round trip flips a floor (the bound's "near an integer" term, continuous: 1e-9 still)
            assert float((own - refs["own"][0]).abs().max()) < 1e-9
        else:
            worst["dccl_lookup own"] = el.ratio(own, *refs["own"])
    # the cross view through the oracle is raw rotated back (combine): compare raw through the combine reference
    cc = el.combine_case(shape, CPU, "real")
    out64 = el.ref_combine(cc)["out"]
    for dt in (torch.float64, torch.float32):
        raw = cc["raw"].to(dt).view(B, H, W, el.CORR_CH).permute(0, 3, 1, 2)
        cross = po.img_rotate(raw, cc["g_back"].to(dt)).permute(0, 2, 3, 1).reshape(-1, el.CORR_CH)
        got = cc["own"].to(dt) + cross
        if dt == torch.float64:
            assert float((got - out64[0]).abs().max()) < 1e-9
        else:
            worst["dccl_combine"] = el.ratio(got, *out64)
    with capsys.disabled():
        print("\nfp32 oracle, worst |err| / bound [%s]: " % shape + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("shape", ["even", "ragged"])
def test_scatter_references_match_float64_autograd(shape):
    B, H, W = el.SHAPES[shape]
    c = el.lookup_bwd_case(shape, CPU, "real")
    refs = el.ref_lookup_bwd(c, launches=1)
    pa = [torch.zeros(B * H * W, 1, H >> i, W >> i, dtype=torch.float64, requires_grad=True) for i in range(4)]
    pb = [torch.zeros(B * H * W, 1, H >> i, W >> i, dtype=torch.float64, requires_grad=True) for i in range(4)]
    # raw (before the rotation back) is what d_raw is the gradient of: differentiate the oracle's lookup with an identity g_back
    ident = po.coords_grid(1, H, W)[0].double()
    own, cross = po.dccl_lookup(c["coords"].double(), pa, pb, c["grid"].double(), ident)
    nchw = lambda t: t.double().view(B, H, W, el.CORR_CH).permute(0, 3, 1, 2)      # noqa: E731
    ((own * nchw(c["d_own"])).sum() + (cross * nchw(c["d_raw"])).sum()).backward()
    for i in range(4):
        assert float((refs[f"g_own{i}"][0] - c["g_own0"][i].double() - pa[i].grad.view(B * H * W, -1)).abs().max()) < 1e-9
        assert float((refs[f"g_other{i}"][0] - c["g_oth0"][i].double() - pb[i].grad.view(B * H * W, -1)).abs().max()) < 1e-7
    cc = el.combine_case(shape, CPU, "real")
    raw = cc["raw"].double().view(B, H, W, el.CORR_CH).permute(0, 3, 1, 2).clone().requires_grad_(True)
    (po.img_rotate(raw, cc["g_back"].double()) * nchw(cc["d_corr"])).sum().backward()
    want = cc["d_raw0"].double() + raw.grad.permute(0, 2, 3, 1).reshape(-1, el.CORR_CH)
    assert float((el.ref_combine_bwd(cc)["d_raw"][0] - want).abs().max()) < 1e-9


def test_pointwise_references_match_float64_autograd():
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1      # noqa: E731
    az, ar, aq, h, dhn = (r(50, 8).requires_grad_(True) for _ in range(5))
    z, rr = torch.sigmoid(az), torch.sigmoid(ar)
    rh = rr * h
    rh.retain_grad()
    q = torch.tanh(aq + 0.5 * rh)
    ((1 - z) * h + z * q).backward(dhn.detach())
    dq = el.ref_gru_q(dhn.detach(), z.detach(), q.detach(), h.detach())
    assert float((dq["dq_pre"][0] - aq.grad).abs().max()) < 1e-12
    zr = el.ref_gru_zr(dq["dz"][0], rh.grad, z.detach(), rr.detach(), h.detach(), dq["dh"][0])
    for a, b in ((zr["dz_pre"][0], az.grad), (zr["dr_pre"][0], ar.grad), (zr["dh"][0], h.grad)):
        assert float((a - b).abs().max()) < 1e-12
    # InstanceNorm + ReLU backward, and the statistics
    B, Np, Cc = 2, 45, 8
    x = (r(B * Np, Cc) * 2).requires_grad_(True)
    dy = r(B * Np, Cc)
    xn = x.view(B, Np, Cc).permute(0, 2, 1)
    torch.relu(torch.nn.functional.instance_norm(xn, eps=el.EPS_NORM)).backward(dy.view(B, Np, Cc).permute(0, 2, 1))
    st = el.ref_stats(x.detach(), B, Np, Cc)
    dx, _ = el.ref_norm_bwd(dy, x.detach(), st["scale"][0], st["shift"][0], True, True, B, Np, Cc)
    assert float((dx - x.grad).abs().max()) < 1e-10
    # frozen BatchNorm
    x = r(33, Cc).requires_grad_(True)
    gamma, beta = (r(Cc) + 2).requires_grad_(True), r(Cc).requires_grad_(True)
    mean, var, dy = r(Cc), r(Cc) + 1.5, r(33, Cc)
    out = torch.relu(torch.nn.functional.batch_norm(x, mean, var, gamma, beta, False, 0.1, 1e-5))
    out.backward(dy)
    ref = el.ref_bn(x.detach(), dy, gamma.detach(), beta.detach(), mean, var, 1e-5, True, None, None, False)
    for a, b in ((ref["out"][0], out.detach()), (ref["dx"][0], x.grad), (ref["dgamma"][0], gamma.grad), (ref["dbeta"][0], beta.grad)):
        assert float((a - b).abs().max()) < 1e-10
    # AdamW against the oracle's fp32 restatement of torch.optim.AdamW, inside the bound.  The entry points take the betas as fp32, so
    # the oracle gets the same fp32 values: 1 - float32(0.999) is 1.3e-5 (relative) off the 1 - 0.999 torch forms in double, which
    # is the C interface's definition of the update and not a rounding of the kernel
    import numpy as np
    f9, f999 = float(np.float32(0.9)), float(np.float32(0.999))
    p, gr = torch.randn(500, generator=g), torch.randn(500, generator=g) * 0.1
    m, v = torch.zeros(500), torch.zeros(500)
    ref, _ = el.ref_adamw(p, gr, m, v, 1e-4, 0.9, 0.999, 1e-8, 5e-5, 1, 1.0)
    wp, wm, wv = po.adamw_step(p.clone(), gr, m.clone(), v.clone(), 1e-4, 1, 5e-5, b1=f9, b2=f999)
    assert el.ratio(wp, *ref["p"]) <= 1.0 and el.ratio(wm, *ref["m"]) <= 1.0 and el.ratio(wv, *ref["v"]) <= 1.0


@pytest.mark.parametrize("shape", ["even", "ragged"])
def test_fp32_oracle_backward_and_pointwise_stay_inside_the_bounds(shape, capsys):
    """Point 4 for the kernels whose fp32 statement is autograd through the oracle, or torch's own fp32 operator: the 'reference
    alone' figure of each.  Absent on purpose: the lookup's cross view and its gradient and motion_prep (the oracle only has them
    composed with a second rotation, whose fp32 rounding no bound here is for), and the sums of channel_stats, norm_bwd with
    instance statistics, bn_frozen_bwd's d gamma / d beta, seq_loss and sum_squares (torch reduces them in fp32, the kernels in
    float64 partials, which is what their bounds describe)."""
    B, H, W = el.SHAPES[shape]
    N, R = H * W, B * H * W
    F = torch.nn.functional
    nchw = lambda t, c: t.view(B, H, W, c).permute(0, 3, 1, 2)                   # noqa: E731
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(R, -1)                         # noqa: E731
    worst = {}
    # lookup_bwd, own view: one launch
    c = el.lookup_bwd_case(shape, CPU, "real")
    refs = el.ref_lookup_bwd(c, launches=1)
    pa = [torch.zeros(R, 1, H >> i, W >> i, requires_grad=True) for i in range(4)]
    pb = [torch.zeros(R, 1, H >> i, W >> i) for i in range(4)]
    own, _ = po.dccl_lookup(c["coords"], pa, pb, c["grid"], po.coords_grid(1, H, W)[0])
    (own * nchw(c["d_own"], el.CORR_CH)).sum().backward()
    worst["dccl_lookup_bwd own"] = max(el.ratio(c["g_own0"][i] + pa[i].grad.view(R, -1), *refs[f"g_own{i}"]) for i in range(4))
    # combine_bwd
    cc = el.combine_case(shape, CPU, "real")
    raw = nchw(cc["raw"], el.CORR_CH).clone().requires_grad_(True)
    (po.img_rotate(raw, cc["g_back"]) * nchw(cc["d_corr"], el.CORR_CH)).sum().backward()
    worst["dccl_combine_bwd"] = el.ratio(cc["d_raw0"] + rows(raw.grad), *el.ref_combine_bwd(cc)["d_raw"])
    # warp_gcorr_bwd
    wc = el.warp_case(shape, CPU, False)
    f1, f2 = nchw(wc["f1"], 256).clone().requires_grad_(True), nchw(wc["f2"], 256).clone().requires_grad_(True)
    (po.warp_groupwise_corr(f1, f2, wc["coords"]) * nchw(wc["d_flaw"], 4)).sum().backward()
    rb = el.ref_warp_bwd(wc)
    worst["warp_gcorr_bwd"] = max(el.ratio(wc["d_f1_0"] + rows(f1.grad), *rb["d_f1"]), el.ratio(wc["d_f2_0"] + rows(f2.grad), *rb["d_f2"]))
    # upsample_flow_bwd
    gen = torch.Generator().manual_seed(7)
    coords1 = (po.coords_grid(B, H, W) + (torch.rand(B, 2, H, W, generator=gen) * 12 - 6)).contiguous()
    mask = torch.rand(R, 576, generator=gen) * 4 - 2
    g = torch.rand(B, 2, 8 * H, 8 * W, generator=gen) * 2 - 1
    d0 = torch.rand(B, 2, H, W, generator=gen) * 2 - 1
    fl = (coords1 - po.coords_grid(B, H, W)).requires_grad_(True)
    mk = nchw(mask, 576).clone().requires_grad_(True)
    (po.upsample_flow(fl, mk) * g).sum().backward()
    ru = el.ref_upsample_bwd(coords1, mask, g, d0, B, H, W)
    worst["upsample_flow_bwd"] = max(el.ratio(rows(mk.grad), *ru["d_mask"]), el.ratio(d0 + fl.grad, *ru["d_flow"]))
    # flow_head_out: torch's fp32 convolution
    x = torch.rand(R, 256, generator=gen) * 2 - 1
    w = torch.rand(2, 9, 256, generator=gen) * 0.1 - 0.05
    bias = torch.rand(2, generator=gen) * 0.2 - 0.1
    rf = el.ref_flow_head(x, w, bias, coords1, B, H, W, 256)
    acc = F.conv2d(nchw(x, 256), w.view(2, 3, 3, 256).permute(0, 3, 1, 2), bias, padding=1)
    worst["flow_head_out"] = max(el.ratio(acc, *rf["delta"]), el.ratio(coords1 + acc, *rf["coords1"]))
    # norm_act and norm_bwd with given scale / shift, frozen BatchNorm forward and dx: fp32 torch and its autograd
    Np, Cc = N, 64
    y = torch.randn(B * Np, Cc, generator=gen).requires_grad_(True)
    res, dy = torch.randn(B * Np, Cc, generator=gen), torch.randn(B * Np, Cc, generator=gen)
    sc, sh = torch.rand(B, Cc, generator=gen) + 0.5, torch.rand(B, Cc, generator=gen) - 0.5
    e = lambda t: t.view(B, 1, Cc)                                                # noqa: E731
    out = torch.relu(res.view(B, Np, Cc) + torch.relu(y.view(B, Np, Cc) * e(sc) + e(sh))).view(-1, Cc)
    worst["norm_act"] = el.ratio(out.detach(), *el.ref_norm_act(y.detach(), sc, sh, B, Np, Cc, res=res))
    torch.relu(y.view(B, Np, Cc) * e(sc) + e(sh)).backward(dy.view(B, Np, Cc))
    worst["norm_bwd fixed"] = el.ratio(y.grad, *el.ref_norm_bwd(dy, y.detach(), sc, sh, True, False, B, Np, Cc))
    xb = torch.randn(459, Cc, generator=gen).requires_grad_(True)
    gam, bet, mean, var = torch.rand(Cc, generator=gen) + 0.5, torch.randn(Cc, generator=gen) * 0.3, torch.randn(Cc, generator=gen) * 0.2, torch.rand(Cc, generator=gen) + 0.3
    dyb = torch.randn(459, Cc, generator=gen)
    ob = torch.relu(F.batch_norm(xb, mean, var, gam, bet, False, 0.1, 1e-5))
    ob.backward(dyb)
    rbn = el.ref_bn(xb.detach(), dyb, gam, bet, mean, var, el.EPS_NORM, True, None, None, False)
    worst["bn_frozen_fwd"] = el.ratio(ob.detach(), *rbn["out"])
    worst["bn_frozen_bwd dx"] = el.ratio(xb.grad, *rbn["dx"])
    # the GRU gate backward: fp32 autograd of the gate arithmetic from the same z, r, q, h
    r_ = lambda lo, hi: (torch.rand(200, 128, generator=gen) * (hi - lo) + lo)   # noqa: E731
    dhn, z, q, h, rr, drh = r_(-1, 1), r_(0.02, 0.98).requires_grad_(True), r_(-0.98, 0.98).requires_grad_(True), r_(-1, 1).requires_grad_(True), r_(0.02, 0.98), r_(-1, 1)
    ((1 - z) * h + z * q).backward(dhn)
    rq = el.ref_gru_q(dhn.double(), z.detach().double(), q.detach().double(), h.detach().double())
    worst["gru_q_bwd"] = max(el.ratio(q.grad * (1 - q.detach() * q.detach()), *rq["dq_pre"]), el.ratio(z.grad, *rq["dz"]), el.ratio(h.grad, *rq["dh"]))
    # AdamW, three steps of the oracle from the state of each
    p, m, v = torch.randn(1031, generator=gen), torch.zeros(1031), torch.zeros(1031)
    import numpy as np
    f9, f999 = float(np.float32(0.9)), float(np.float32(0.999))
    worst["adamw_step"] = 0.0
    for k in range(3):
        gk = torch.randn(1031, generator=gen) * 0.1
        ra, _ = el.ref_adamw(p, gk, m, v, 1e-4, 0.9, 0.999, 1e-8, 5e-5, k + 1, 1.0)
        p, m, v = po.adamw_step(p, gk, m, v, 1e-4, k + 1, 5e-5, b1=f9, b2=f999)
        worst["adamw_step"] = max(worst["adamw_step"], el.ratio(p, *ra["p"]), el.ratio(m, *ra["m"]), el.ratio(v, *ra["v"]))
    with capsys.disabled():
        print("\nfp32 oracle / torch, worst |err| / bound [%s]: " % shape + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("shape", ["even", "ragged"])
def test_warp_rotate_upsample_references_match_the_oracle(shape, capsys):
    """The remaining gathers and their backward against the oracle in float64 (values) and through float64 autograd (scatters);
    the fp32 oracle inside the bounds."""
    B, H, W = el.SHAPES[shape]
    N = H * W
    nchw = lambda t, c: t.view(B, H, W, c).permute(0, 3, 1, 2)                   # noqa: E731
    worst = {}
    c = el.warp_case(shape, CPU, False)
    _, _, ref, bnd = el.ref_warp(c)
    f1 = nchw(c["f1"].double(), 256).clone().requires_grad_(True)
    f2 = nchw(c["f2"].double(), 256).clone().requires_grad_(True)
    got = po.warp_groupwise_corr(f1, f2, c["coords"].double())
    assert float((got.detach().permute(0, 2, 3, 1).reshape(-1, 4) - ref).abs().max()) < 1e-9
    (got * nchw(c["d_flaw"].double(), 4)).sum().backward()
    refb = el.ref_warp_bwd(c)
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(B * N, -1)                     # noqa: E731
    assert float((refb["d_f1"][0] - c["d_f1_0"].double() - rows(f1.grad)).abs().max()) < 1e-9
    assert float((refb["d_f2"][0] - c["d_f2_0"].double() - rows(f2.grad)).abs().max()) < 1e-9
    got32 = po.warp_groupwise_corr(nchw(c["f1"], 256), nchw(c["f2"], 256), c["coords"])
    worst["warp_gcorr"] = el.ratio(rows(got32), ref, bnd)
    # flo_rotate: away from the jumps the bound flags (there the oracle, rounded in float64, may take the other branch)
    gen = torch.Generator().manual_seed(2)
    g_w2c, g_c2w = el.rotate_grids(H, W, "real", gen, CPU)
    flow = el.edge_flows(f"el/rot/{shape}", B, H, W, gen)
    ref, bnd = el.ref_flo_rotate(flow, g_w2c, g_c2w)
    smooth = bnd < 1e-2
    assert float(smooth.double().mean()) > 0.9
    got = po.flo_rotate(flow.double(), g_w2c.double(), g_c2w.double())
    assert float(((got - ref).abs() * smooth).max()) < 1e-8
    worst["flo_rotate"] = el.ratio(po.flo_rotate(flow, g_w2c, g_c2w), ref, bnd)
    # convex upsampling and its backward
    fl = (torch.rand(B, 2, H, W, generator=gen) * 12 - 6)
    coords1 = (po.coords_grid(B, H, W) + fl).contiguous()
    mask = torch.rand(B * N, 576, generator=gen) * 4 - 2
    g = torch.rand(B, 2, 8 * H, 8 * W, generator=gen) * 2 - 1
    ref, bnd = el.ref_upsample(coords1, mask, B, H, W)
    f64 = (coords1 - po.coords_grid(B, H, W)).double().requires_grad_(True)      # the flow the kernel forms, upcast
    m64 = nchw(mask.double(), 576).clone().requires_grad_(True)
    up = po.upsample_flow(f64, m64)
    assert float((up.detach() - ref).abs().max()) < 1e-9
    (up * g.double()).sum().backward()
    d0 = torch.zeros(B, 2, H, W)
    refb = el.ref_upsample_bwd(coords1, mask, g, d0, B, H, W)
    assert float((refb["d_mask"][0] - rows(m64.grad)).abs().max()) < 1e-9
    assert float((refb["d_flow"][0] - f64.grad).abs().max()) < 1e-9
    worst["upsample_flow"] = el.ratio(po.upsample_flow(coords1 - po.coords_grid(B, H, W), nchw(mask, 576)), ref, bnd)
    # the pyramid's backward through the oracle's build_pyramid
    R = N
    v = torch.rand(1, H, W, H, W, generator=gen, dtype=torch.float64).requires_grad_(True)
    pyr = po.build_pyramid(v)
    gl = [torch.rand(p.shape, generator=gen) for p in pyr]
    sum((p * q.double()).sum() for p, q in zip(pyr, gl)).backward()
    refp, _ = el.ref_pyramid_bwd([q.reshape(R, -1) for q in gl], H, W)
    assert float((refp - v.grad.reshape(R, -1)).abs().max()) < 1e-12
    # the sequence loss: the oracle's loss and gradient for one prediction
    pred, gt = torch.randn(B, 2, H, W, generator=gen) * 3, torch.randn(B, 2, H, W, generator=gen) * 3
    valid = (torch.rand(B, H, W, generator=gen) > 0.3).float()
    loss, metrics, grads = po.uniform_loss([pred], gt, valid)
    rl = el.ref_seq_loss(pred, gt, valid, po.spherical_mask(H, W).reshape(-1), 1.0, 400.0, 5)
    tot = rl["partials"][0].sum((0, 1))
    assert abs(float(tot[0]) - loss) < 1e-6 * abs(loss) and abs(float(tot[1] / tot[2]) - metrics["epe"]) < 1e-6
    assert abs(float(tot[3] / tot[2]) - metrics["1px"]) < 1e-12
    worst["seq_loss grad"] = el.ratio(grads[0], *rl["grad"])
    with capsys.disabled():
        print("\nfp32 oracle, worst |err| / bound [%s]: " % shape + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst


def test_dropped_tap_fails_the_other_gathers():
    c = el.warp_case("ragged", CPU, True)
    good, bad = el.ref_warp(c), el.ref_warp(c, mut="drop_tap")
    assert failed(bad[2], good[2], good[3])
    gen = torch.Generator().manual_seed(2)
    B, H, W = el.SHAPES["ragged"]
    g_w2c, g_c2w = el.rotate_grids(H, W, "real", gen, CPU)
    flow = el.edge_flows("el/rot/ragged", B, H, W, gen)
    ref, bnd = el.ref_flo_rotate(flow, g_w2c, g_c2w)
    assert failed(el.ref_flo_rotate(flow, g_w2c, g_c2w, mut="drop_tap")[0], ref, bnd)



# ------------------------------------------------------------------------------------------------------------------------
# 3. deliberate mistakes, applied to the reference output, fail the bound of their kernel
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mut,shape", [("drop_tap", "even"), ("origin_off", "even"), ("ceil_width", "ragged"), ("seam_off", "even"),
                                       ("seam_off", "folded")])
def test_gather_mistakes_fail_the_lookup_bound(mut, shape):
    c = el.lookup_case(shape, CPU, "real")
    good, bad = el.ref_lookup(c), el.ref_lookup(c, mut=mut)
    assert failed(bad["own"][0], *good["own"]), "own view"
    assert failed(bad["raw"][0], *good["raw"]), "cross view"
    if mut == "drop_tap":
        cc = el.combine_case(shape, CPU, "real")
        assert failed(el.ref_combine(cc, mut=mut)["out"][0], *el.ref_combine(cc)["out"])


def test_ceil_width_is_the_floor_width_on_even_maps():
    """The mistake exists only where W / 2^l is not an integer: the ragged map is what catches it."""
    assert [el.level_dims(16, 32, l, "ceil_width") for l in range(4)] == [el.level_dims(16, 32, l) for l in range(4)]
    assert [el.level_dims(17, 27, l, "ceil_width")[1] for l in range(4)] == [27, 14, 7, 4]
    assert [el.level_dims(17, 27, l) for l in range(4)] == [(17, 27), (8, 13), (4, 6), (2, 3)]


def test_scatter_mistakes_fail_the_lookup_bwd_bound():
    c = el.lookup_bwd_case("ragged", CPU, "real")
    good = el.ref_lookup_bwd(c)
    for mut in ("lose_second", "drop_tap"):
        bad = el.ref_lookup_bwd(c, mut=mut)
        for lvl in range(4):
            assert failed(bad[f"g_own{lvl}"][0], *good[f"g_own{lvl}"]), (mut, lvl)
            assert failed(bad[f"g_other{lvl}"][0], *good[f"g_other{lvl}"]), (mut, lvl)
    # a clear_raw that leaves one row: the cleared buffer is compared exactly
    left = torch.zeros_like(c["d_raw"])
    left[-1] = c["d_raw"][-1]
    assert failed(left, torch.zeros_like(left, dtype=torch.float64), 0.0)
    cc = el.combine_case("ragged", CPU, "real")
    assert failed(el.ref_combine_bwd(cc, launches=2)["d_raw"][0], *el.ref_combine_bwd(cc)["d_raw"])


@pytest.mark.parametrize("Np,nblk", [(459, 128), (240, 7), (96, 96)])
def test_reduction_mistakes_fail_their_bounds(Np, nblk):
    B, Cc = 2, 64
    g = torch.Generator().manual_seed(Np)
    y, dy = torch.randn(B * Np, Cc, generator=g) + 0.5, torch.randn(B * Np, Cc, generator=g)
    good = el.ref_stats(y, B, Np, Cc)
    for mut in ("drop_chunk", "unbiased"):
        bad = el.ref_stats(y, B, Np, Cc, mut=mut, nblk=nblk)
        assert failed(bad["scale"][0], *good["scale"]), mut
    assert failed(el.ref_stats(y, B, Np, Cc, mut="drop_chunk", nblk=nblk)["shift"][0], *good["shift"])
    s, t = good["scale"][0].float(), good["shift"][0].float()
    assert failed(el.ref_norm_bwd(dy, y, s, t, True, True, B, Np, Cc, mut="drop_chunk", nblk=nblk)[0],
                  *el.ref_norm_bwd(dy, y, s, t, True, True, B, Np, Cc))
    one = torch.ones(Cc)
    args = (y, dy, one, 0 * one, 0 * one, one, 1e-5, True, None, None, False)
    goodb, badb = el.ref_bn(*args), el.ref_bn(*args, mut="drop_chunk", nblk=max(1, min(B * Np // 16, 2048)))
    assert failed(badb["dgamma"][0], *goodb["dgamma"]) and failed(badb["dbeta"][0], *goodb["dbeta"])
    pred, gt = torch.randn(2, 2, 17, 27, generator=g), torch.randn(2, 2, 17, 27, generator=g)
    valid, w = torch.ones(2, 17, 27), torch.ones(17 * 27)
    goods, bads = el.ref_seq_loss(pred, gt, valid, w, 0.8, 400.0, 7), el.ref_seq_loss(pred, gt, valid, w, 0.8, 400.0, 7, mut="drop_chunk")
    assert failed(bads["partials"][0], *goods["partials"])


def test_swapped_gate_fails_the_gru_bound():
    g = torch.Generator().manual_seed(4)
    r = lambda lo, hi: torch.rand(200, 128, generator=g, dtype=torch.float64) * (hi - lo) + lo      # noqa: E731
    a = (r(-1, 1), r(0.02, 0.98), r(-0.98, 0.98), r(-1, 1))
    good, bad = el.ref_gru_q(*a), el.ref_gru_q(*a, mut="swap_z")
    assert failed(bad["dq_pre"][0], *good["dq_pre"]) and failed(bad["dh"][0], *good["dh"])
