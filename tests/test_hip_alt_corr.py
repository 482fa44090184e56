"""alternate_corr on the MI355X: pf_feature_pyramid and pf_dccl_lookup_feat against float64 restatements
(tests/alt_corr_ref.py) and against pf_dccl_lookup on the product's volume pyramids, then the forward with
``args.alternate_corr`` against the goldens, the CPU oracle and the default mode, its memory footprint up to a 1920x3840
panorama, and the flag's hygiene.  Run with ``-m gpu``."""
import argparse
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import alt_corr_ref as ref
import golden_cases as gc
import priorflow_oracle as po

pytestmark = pytest.mark.gpu
T = torch.from_numpy
EPE_BAR = 1e-3
EPS = float(torch.finfo(torch.float32).eps)
# pf_lookup_feat_kernel's worst case per value, in fp32 eps x sum_j w_j sum_c |f1 P_i(f2)| / sqrt(C): 8 FMAs per lane and a
# 6-level butterfly (14), three pooling levels (9), the bilinear sum (4); rounded up
K_FEAT = 32


@pytest.fixture(scope="module")
def lib():
    from prior_flow_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def params():
    from prior_flow_amd.modules import state_dict_shapes
    return gc.det_state_dict(state_dict_shapes())


def make_model(params, **args):
    from prior_flow_amd.prior_raft import PriOr_RAFT
    m = PriOr_RAFT(argparse.Namespace(**dict(dict(mixed_precision=False, dropout=0.0), **args)))
    m.load_state_dict(params, strict=True)
    return m.cuda().eval()


@pytest.fixture(scope="module")
def model(params):
    return make_model(params, alternate_corr=True)


def epe(a, b):
    b = b if isinstance(b, torch.Tensor) else T(np.asarray(b))
    e = po.epe(a.detach().cpu().float(), b.detach().cpu().float())
    return float(e.mean()), float(e.max())


# ---- kernels --------------------------------------------------------------------------------------------------------
def _grid(h, w):
    return po.sample_grid(h, w, po.rotation_x(math.pi / 2)).contiguous()


def _coords(kind, tag, B, h, w):
    xs = torch.arange(w).view(1, 1, w).expand(B, h, w).float()
    ys = torch.arange(h).view(1, h, 1).expand(B, h, w).float()
    c0 = torch.stack([xs, ys], 1).contiguous()
    if kind == "zero":
        return c0
    if kind == "large":                                  # flows of tens of pixels: scattered corners, many out of range
        return (c0 + gc.uni(tag + "/large", (B, 2, h, w), -40.0, 40.0)).contiguous()
    return gc.nasty_coords(tag, B, h, w)


def _feat_levels(lib, f2_rows, B, h, w):
    lv = [torch.empty(B * (h >> i) * (w >> i), f2_rows.shape[1], device=f2_rows.device) for i in (1, 2, 3)]
    lib.feature_pyramid(f2_rows, lv, B, h, w)
    return [f2_rows] + lv


def _run_feat(lib, coords, f1a, f2a, f1b, f2b, g, ld=324, fill=0.0, counts=None):
    dev = torch.device("cuda")
    B, _, h, w = f1a.shape
    ra, rb = ref.rows(f1a).to(dev), ref.rows(f1b).to(dev)
    la, lb = _feat_levels(lib, ref.rows(f2a).to(dev), B, h, w), _feat_levels(lib, ref.rows(f2b).to(dev), B, h, w)
    own = torch.full((B * h * w, ld), fill, device=dev)
    raw = torch.full((B * h * w, ld), fill, device=dev)
    lib.dccl_lookup_feat(coords.to(dev).contiguous(), ra, la, rb, lb, g.to(dev), own, raw, counts)
    torch.cuda.synchronize()
    return own, raw


def _units(B, h, w):
    """(tile, level, view) units of one launch: 2 x 4 pixel tiles per image, 4 levels, 2 views."""
    return B * ((h + 1) // 2) * ((w + 3) // 4) * 4 * 2


def _check(got, want, mag, k, what):
    err = (got.double().cpu() - want.cpu()).abs()
    bound = k * EPS * mag.cpu()
    worst = float((err / (bound + 1e-30)).max())
    assert bool((err <= bound).all()), f"{what}: worst err / bound {worst:.3g}"
    return worst


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("hw", [(16, 32), (20, 44), (16, 40)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_feature_pyramid_matches_avg_pool2d(lib, hw, B):
    h, w = hw
    _, f2 = gc.fmaps(f"altcorr/pool/{h}x{w}", B, h, w)
    lv = _feat_levels(lib, ref.rows(f2).cuda(), B, h, w)
    cur = f2.cuda()
    for i in (1, 2, 3):
        cur = F.avg_pool2d(cur, 2)
        assert tuple(lv[i].shape) == (B * cur.shape[-2] * cur.shape[-1], f2.shape[1])
        torch.testing.assert_close(lv[i], ref.rows(cur), rtol=0, atol=8 * EPS * 1.7)


@pytest.mark.parametrize("coords_kind", ["nasty", "zero", "large"])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("hw", [(16, 32), (20, 44), (16, 40)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_lookup_feat_matches_float64(lib, hw, B, coords_kind):
    h, w = hw
    tag = f"altcorr/{h}x{w}/{B}"
    f1a, f2a = gc.fmaps(tag + "/a", B, h, w)
    f1b, f2b = gc.fmaps(tag + "/b", B, h, w)
    coords, g = _coords(coords_kind, tag, B, h, w), _grid(h, w)
    counts = torch.zeros(2, dtype=torch.int32, device="cuda")
    own, raw = _run_feat(lib, coords, f1a, f2a, f1b, f2b, g, counts=counts)
    tiled, pixel = (int(v) for v in counts.cpu())
    print(f"{coords_kind}: {tiled} tile-path units, {pixel} pixel-path units")
    assert tiled + pixel == _units(B, h, w)
    assert tiled > 0 and pixel > 0          # seam tiles (x wraps mod W_i) always take the pixel path
    w_own, w_raw = ref.lookup_feat(coords, f1a, f2a, f1b, f2b, g)
    m_own, m_raw = ref.lookup_feat(coords, f1a, f2a, f1b, f2b, g, absolute=True)
    _check(own, w_own, m_own, K_FEAT, "own")
    _check(raw, w_raw, m_raw, K_FEAT, "raw")


@pytest.mark.parametrize("B,hw", [(2, (64, 128)), (1, (80, 160))], ids=["64x128_b2", "80x160"])
def test_lookup_feat_matches_volume_lookup(lib, B, hw):
    """Against the default mode's own kernels: pf_dccl_lookup on pf_corr_pyramid (fp32) and pf_corr_pyramid_bf16x3."""
    from prior_flow_amd.engine import split_twin
    h, w = hw
    dev = torch.device("cuda")
    tag = f"altcorr/vol/{h}x{w}"
    f1a, f2a = gc.fmaps(tag + "/a", B, h, w)
    f1b, f2b = gc.fmaps(tag + "/b", B, h, w)
    coords, g = _coords("nasty", tag, B, h, w), _grid(h, w)
    gd, cd = g.to(dev), coords.to(dev)
    own, raw = _run_feat(lib, coords, f1a, f2a, f1b, f2b, g)
    m_own, m_raw = ref.lookup_feat(cd, f1a.to(dev), f2a.to(dev), f1b.to(dev), f2b.to(dev), gd, absolute=True)
    N = h * w
    rows = {k: ref.rows(v).to(dev) for k, v in (("f1a", f1a), ("f2a", f2a), ("f1b", f1b), ("f2b", f2b))}
    pyr = lambda: [torch.empty(B * N, (h >> i) * (w >> i), device=dev) for i in range(4)]  # noqa: E731
    for form, k in (("fp32", 64), ("bf16x3", 2.0 ** -14 / EPS)):
        pa, pb = pyr(), pyr()
        if form == "fp32":
            lib.corr_pyramid(rows["f1a"], rows["f2a"], pa, B, h, w)
            lib.corr_pyramid(rows["f1b"], rows["f2b"], pb, B, h, w)
        else:
            tw = {}
            for key, r in rows.items():
                tw[key] = split_twin(B * N, 256, dev)
                lib.split_bf16(r, tw[key])
            lib.corr_pyramid_bf16x3(tw["f1a"], tw["f2a"], pa, B, h, w, 256)
            lib.corr_pyramid_bf16x3(tw["f1b"], tw["f2b"], pb, B, h, w, 256)
        v_own, v_raw = torch.empty(B * N, 324, device=dev), torch.empty(B * N, 324, device=dev)
        lib.dccl_lookup(cd, pa, pb, gd, v_own, v_raw)
        torch.cuda.synchronize()
        print(f"{form}: own {_check(own, v_own.double(), m_own, k, form + ' own'):.3f} "
              f"raw {_check(raw, v_raw.double(), m_raw, k, form + ' raw'):.3f} of the bound")
        del pa, pb
    # both paths ran in the launch above, and each path alone matches as well: zero flow keeps the interior on the tile path
    counts = torch.zeros(2, dtype=torch.int32, device=dev)
    _run_feat(lib, coords, f1a, f2a, f1b, f2b, g, counts=counts)
    assert int(counts[0]) > 0 and int(counts[1]) > 0 and int(counts.sum()) == _units(B, h, w)
    c0 = _coords("zero", tag, B, h, w)
    counts.zero_()
    z_own, z_raw = _run_feat(lib, c0, f1a, f2a, f1b, f2b, g, counts=counts)
    assert int(counts[0]) > 4 * int(counts[1]), counts
    z_ref = ref.lookup_feat(c0.to(dev), f1a.to(dev), f2a.to(dev), f1b.to(dev), f2b.to(dev), gd, absolute=True)
    pa, pb = pyr(), pyr()
    lib.corr_pyramid(rows["f1a"], rows["f2a"], pa, B, h, w)
    lib.corr_pyramid(rows["f1b"], rows["f2b"], pb, B, h, w)
    v_own, v_raw = torch.empty(B * N, 324, device=dev), torch.empty(B * N, 324, device=dev)
    lib.dccl_lookup(c0.to(dev), pa, pb, gd, v_own, v_raw)
    _check(z_own, v_own.double(), z_ref[0], 64, "zero flow own")
    _check(z_raw, v_raw.double(), z_ref[1], 64, "zero flow raw")
    del pa, pb
    # padded row stride: columns 324..335 untouched, values bitwise those of ld = 324
    own2, raw2 = _run_feat(lib, coords, f1a, f2a, f1b, f2b, g, ld=336, fill=7.0)
    assert torch.equal(own2[:, :324], own) and torch.equal(raw2[:, :324], raw)
    assert bool((own2[:, 324:] == 7.0).all()) and bool((raw2[:, 324:] == 7.0).all()), "padding columns must stay untouched"
    # two launches: bitwise equal
    own3, raw3 = _run_feat(lib, coords, f1a, f2a, f1b, f2b, g)
    assert torch.equal(own3, own) and torch.equal(raw3, raw)
    if B == 2:        # image b of a B = 2 launch: bitwise the B = 1 launch
        one = lambda t: t[1:].contiguous()  # noqa: E731
        own1, raw1 = _run_feat(lib, one(coords), one(f1a), one(f2a), one(f1b), one(f2b), g)
        assert torch.equal(own1, own[N:]) and torch.equal(raw1, raw[N:])


def test_lookup_feat_4k_geometry_sampled(lib):
    """1920x3840 (240 x 480 at 1/8): 512 sampled pixels, seam and pole pixels among them, all 324 channels of both outputs."""
    B, h, w, C = 1, 240, 480, 256
    gen = torch.Generator().manual_seed(4096)
    f1a, f2a, f1b, f2b = (torch.rand(B, C, h, w, generator=gen) * 3.4 - 1.7 for _ in range(4))
    c0 = _coords("zero", "", B, h, w)
    coords = (c0 + (torch.rand(B, 2, h, w, generator=gen) * 24 - 12)).contiguous()
    g = _grid(h, w)
    own, raw = _run_feat(lib, coords, f1a, f2a, f1b, f2b, g)
    special = [y * w + x for y in (0, 1, h // 2, h - 2, h - 1) for x in (0, 1, w // 2, w - 2, w - 1)]
    pix = torch.cat([torch.tensor(special), torch.randint(0, h * w, (512 - len(special),), generator=gen)])
    # the restatement's fp32 geometry runs on the host, where the oracle pins it (pixel -> [-1, 1] -> pixel round trip and
    # remainder as ATen's CPU kernels round them): a one-ulp shift of a tap moves a value by ~1e-4 at this width
    w_own, w_raw = ref.lookup_feat(coords, f1a, f2a, f1b, f2b, g, pix)
    m_own, m_raw = ref.lookup_feat(coords, f1a, f2a, f1b, f2b, g, pix, absolute=True)
    _check(own[pix.cuda()], w_own, m_own, K_FEAT, "own (4K)")
    _check(raw[pix.cuda()], w_raw, m_raw, K_FEAT, "raw (4K)")
    assert float(w_raw.abs().max()) > 0.1 and float(w_own.abs().max()) > 0.1


# ---- forward --------------------------------------------------------------------------------------------------------
def test_forward_alternate_matches_golden_lists_and_test_mode(model):
    i1, i2 = gc.synthetic_pair(1, 128, 256)
    g = gc.load("forward_128x256_it12")
    sub = lambda t: t[:, :, ::2, ::2]  # noqa: E731
    with torch.no_grad():
        pa, pb = model(i1.cuda(), i2.cuda(), iters=12)
        flow = model(i1.cuda(), i2.cuda(), iters=12, test_mode=True)
    assert model._ws and all(ws.alt_corr and ws.pyr_a is None for ws in model._ws.values())
    for i in (0, 2, 6):
        assert epe(sub(pa[i]), g[f"a{i}"])[0] < EPE_BAR
        assert epe(sub(pb[i]), g[f"b{i}"])[0] < EPE_BAR
    for pred, key in ((pa[11], "a11"), (pb[11], "b11"), (flow, "a11")):
        mean, mx = epe(pred, g[key])
        print(f"alternate_corr {key}: mean EPE {mean:.3e} max {mx:.3e}")
        assert mean < EPE_BAR, (key, mean, mx)


def test_forward_alternate_exact_fp32(params):
    from prior_flow_amd._lib import PREC_F32
    m = make_model(params, alternate_corr=True)
    m.precision = PREC_F32
    i1, i2 = gc.synthetic_pair(1, 128, 256)
    with torch.no_grad():
        out = m(i1.cuda(), i2.cuda(), iters=12, test_mode=True)
    mean, mx = epe(out, gc.load("forward_128x256_it12")["a11"])
    print(f"alternate_corr + exact fp32: mean EPE {mean:.3e} max {mx:.3e}")
    assert mean < 2e-5, (mean, mx)


def test_forward_alternate_eager_equals_graph(model):
    i1, i2 = gc.synthetic_pair(1, 128, 256, seed=5)
    with torch.no_grad():
        model.use_graph = False
        eager = model(i1.cuda(), i2.cuda(), iters=12, test_mode=True)
        model.use_graph = True
        g1 = model(i1.cuda(), i2.cuda(), iters=12, test_mode=True)
        g2 = model(i1.cuda(), i2.cuda(), iters=12, test_mode=True)
    assert torch.equal(g1, g2), "graph replay must be deterministic"
    assert torch.equal(g1, eager), "graph replay differs from eager launches"


def test_forward_alternate_init_flow_and_batch2(model):
    i1, i2 = gc.synthetic_pair(1, 128, 256)
    init = gc.uni("fwd/init_flow", (1, 2, 16, 32), -3, 3).cuda()
    with torch.no_grad():
        out = model(i1.cuda(), i2.cuda(), iters=3, init_flow=init, test_mode=True)
    assert epe(out, gc.load("forward_128x256_init")["out"])[0] < EPE_BAR
    j1, j2 = gc.synthetic_pair(2, 128, 256, seed=77)
    with torch.no_grad():
        out = model(j1.cuda(), j2.cuda(), iters=2, test_mode=True)
        solo = model(j1[1:].cuda(), j2[1:].cuda(), iters=2, test_mode=True)
    assert epe(out[:, :, ::2, ::2], gc.load("forward_128x256_b2")["out"])[0] < EPE_BAR
    assert epe(solo, out[1:])[0] < 1e-5


def test_forward_alternate_512x1024_vs_oracle(model, params):
    i1, i2 = gc.synthetic_pair(1, 512, 1024)
    with torch.no_grad():
        out = model(i1.cuda(), i2.cuda(), iters=12, test_mode=True)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    ref_flow = po.forward(params, i1, i2, iters=12, test_mode=True)
    mean, mx = epe(out, ref_flow)
    print(f"alternate_corr 512x1024 vs CPU oracle: mean EPE {mean:.3e} max {mx:.3e}")
    assert mean < EPE_BAR, (mean, mx)


# ---- memory ---------------------------------------------------------------------------------------------------------
def test_memory_512x1024_then_4k_panorama(params, lib):
    from prior_flow_amd.engine import Workspace
    dev = torch.device("cuda")
    H, W = 512, 1024
    N = (H // 8) * (W // 8)
    ws = Workspace(lib, 1, H, W, dev, alt_corr=True)
    tensors = [t for v in vars(ws).values() for t in (v if isinstance(v, (list, tuple)) else
                                                      (v.values() if isinstance(v, dict) else [v])) if isinstance(t, torch.Tensor)]
    assert tensors and max(t.numel() for t in tensors) < N * N, "a workspace tensor as large as a correlation volume"
    alt_bytes = ws.nbytes()
    del ws, tensors
    ws = Workspace(lib, 1, H, W, dev)
    default_bytes = ws.nbytes()
    del ws
    print(f"512x1024 workspace: {default_bytes / 2**30:.3f} GiB default, {alt_bytes / 2**30:.3f} GiB alternate_corr")
    assert default_bytes - alt_bytes >= 0.7e9
    # one 1920x3840 panorama (the default mode would need 141 GB for its two pyramids)
    m = make_model(params, alternate_corr=True)
    torch.cuda.empty_cache()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    gen = torch.Generator().manual_seed(3840)
    i1 = (torch.rand(1, 3, 1920, 3840, generator=gen) * 255).cuda()
    i2 = torch.roll(i1, shifts=(3, 11), dims=(2, 3))
    with torch.no_grad():
        out = m(i1, i2, iters=12, test_mode=True)
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - base
    print(f"1920x3840 B=1 iters=12 alternate_corr: peak allocation growth {grew / 2**30:.2f} GiB")
    assert tuple(out.shape) == (1, 2, 1920, 3840) and bool(torch.isfinite(out).all())
    assert grew < 48 * 2**30
    del m, out
    torch.cuda.empty_cache()


# ---- flag hygiene ---------------------------------------------------------------------------------------------------
def test_switching_the_flag_off_restores_the_default_path(params):
    i1, i2 = gc.synthetic_pair(1, 128, 256, seed=9)
    m = make_model(params)
    with torch.no_grad():
        default = m(i1.cuda(), i2.cuda(), iters=4, test_mode=True)
        graphs = dict(m._graphs)                         # (held: the objects stay distinct from any new capture)
        m.alternate_corr = True
        alt = m(i1.cuda(), i2.cuda(), iters=4, test_mode=True)
        assert all(ws.alt_corr for ws in m._ws.values()) and len(m._ws) == 1
        assert graphs and all(m._graphs.get(k) is not g for k, g in graphs.items()), "graphs of the other mode must be gone"
        m.alternate_corr = None                          # follow args (False)
        back = m(i1.cuda(), i2.cuda(), iters=4, test_mode=True)
        fresh = make_model(params)(i1.cuda(), i2.cuda(), iters=4, test_mode=True)
    assert all(not ws.alt_corr for ws in m._ws.values())
    assert torch.equal(back, fresh) and torch.equal(default, fresh)
    assert not torch.equal(alt, fresh)                   # a different arithmetic: equal only up to rounding
    assert epe(alt, fresh)[0] < EPE_BAR


def test_mixed_precision_with_alternate_corr(params):
    i1, i2 = gc.synthetic_pair(1, 512, 1024)
    with torch.no_grad():
        mixed = make_model(params, mixed_precision=True)(i1.cuda(), i2.cuda(), iters=12, test_mode=True)
        both = make_model(params, mixed_precision=True, alternate_corr=True)(i1.cuda(), i2.cuda(), iters=12, test_mode=True)
    assert torch.isfinite(both).all()
    mean, mx = epe(both, mixed)
    print(f"mixed_precision + alternate_corr vs mixed_precision: mean EPE {mean:.3e} max {mx:.3e}")
    assert mean < EPE_BAR, (mean, mx)


def test_training_forward_refuses_the_flag(params):
    from prior_flow_amd._lib import PfError
    m = make_model(params, alternate_corr=True)
    m.train()
    i1, i2 = gc.synthetic_pair(1, 128, 256)
    with pytest.raises(PfError, match="inference-only"):
        m(i1.cuda(), i2.cuda(), iters=2)
