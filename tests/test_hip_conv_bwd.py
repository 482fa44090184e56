"""Convolution backward building blocks (SURVEY.md 8f-3 groundwork) against torch autograd on the CPU:
pf_conv2d_wgrad (weight + bias gradient, transposed-LDS-read MFMA kernel) and the data gradient through
pf_conv2d on flipped / transposed weights (engine.Conv.dgrad_of).  Further down, directed cases of both weight-gradient kernels
against float64 under the derived bounds of tests/wgrad_launches.py: splits / workgroups that own several pixel tiles."""
import pytest
import torch

import golden_cases as gc
import kernel_cases as kc
import wgrad_launches as wl

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from prior_flow_amd import _lib
    return _lib.load()


CASES = [  # kh, kw, c0, c1, cout, B, H, W
    (3, 3, 64, 0, 64, 2, 8, 32),
    (3, 3, 128, 0, 256, 1, 16, 64),
    (1, 5, 128, 256, 256, 1, 16, 32),          # GRU gates: [h | x] virtual concat
    (5, 1, 128, 256, 128, 2, 12, 32),
    (1, 1, 324, 0, 256, 1, 16, 32),            # convc1: ragged channel tail
    (3, 3, 72, 0, 126, 2, 7, 45),              # partial tiles, Cout not a tile multiple (126 % 4 != 0 -> 128 padded)
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_wgrad_and_dgrad_vs_autograd(lib, case):
    from prior_flow_amd._lib import EPI_LINEAR, PREC_BF16X3
    from prior_flow_amd.engine import Conv
    kh, kw, c0, c1, cout, B, H, W = case
    dev = torch.device("cuda")
    cin = c0 + c1
    tag = "bw/" + "x".join(map(str, case))
    x = gc.uni(tag + "/x", (B, cin, H, W), -1, 1).requires_grad_(True)
    w = gc.uni(tag + "/w", (cout, cin, kh, kw), -0.1, 0.1).requires_grad_(True)
    b = gc.uni(tag + "/b", (cout,), -0.1, 0.1).requires_grad_(True)
    gy = gc.uni(tag + "/gy", (B, cout, H, W), -1, 1)
    y = torch.nn.functional.conv2d(x, w, b, padding=(kh // 2, kw // 2))
    (y * gy).sum().backward()
    # device buffers: activations and dY live in wider row buffers (column offsets like the engine's)
    cpad = (cout + 3) // 4 * 4
    dy = torch.zeros(B * H * W, cpad + 8, device=dev)
    dy[:, 4:4 + cout] = kc.cl(gy).to(dev)
    x0 = torch.full((B * H * W, c0 + 4), 3.0, device=dev)
    x0[:, :c0] = kc.cl(x.detach()[:, :c0]).to(dev)
    x1 = None
    if c1:
        x1 = torch.full((B * H * W, c1 + 8), -2.0, device=dev)
        x1[:, 8:8 + c1] = kc.cl(x.detach()[:, c0:]).to(dev)
    cin_pad, cout_pad = (cin + 31) // 32 * 32, (cout + 127) // 128 * 128
    dw = torch.zeros(cout_pad, kh * kw, cin_pad, device=dev)
    db = torch.zeros(cout_pad, device=dev)
    lib.conv2d_wgrad(x0, 0, c0, dy, 4, cpad, dw, db, kh, kw, B, H, W, x1=x1, off1=8, c1=c1)
    got_w = Conv.unpack_wgrad(dw, cout, cin, kh, kw).cpu()
    scale = float(w.grad.abs().max())
    kc.check(got_w, w.grad, 3e-5 * scale + 1e-6, "weight gradient")
    kc.check(db[:cout], b.grad, 3e-5 * float(b.grad.abs().max()) + 1e-6, "bias gradient")
    assert float(dw[cout:].abs().max() if cout < cout_pad else 0.0) == 0.0 and float(dw[:, :, cin:].abs().max() if cin < cin_pad else 0.0) == 0.0
    # accumulation semantics: a second call doubles
    lib.conv2d_wgrad(x0, 0, c0, dy, 4, cpad, dw, None, kh, kw, B, H, W, x1=x1, off1=8, c1=c1)
    kc.check(Conv.unpack_wgrad(dw, cout, cin, kh, kw).cpu(), 2 * w.grad, 6e-5 * scale + 2e-6, "weight gradient accumulates")
    # data gradient through the forward kernel
    if cout % 4 == 0:
        dg = Conv.dgrad_of(w.detach().to(dev), PREC_BF16X3)
        dx = torch.empty(B * H * W, cin, device=dev)
        lib.conv2d([dg.desc(dy, 4, cout, dx, 0, EPI_LINEAR)], B, H, W, dy)
        kc.check(kc.uncl(dx.cpu(), B, H, W), x.grad, 2e-4 * float(x.grad.abs().max()), "data gradient")


@pytest.mark.parametrize("case", [(3, 64, 7, 2, 2, 36, 52), (2, 128, 7, 1, 2, 17, 27), (4, 64, 3, 1, 1, 9, 10)],
                         ids=lambda c: "x".join(map(str, c)))
def test_small_cin_wgrad_vs_autograd(lib, case):
    """pf_conv2d_wgrad_small (the 7x7 stems' weight / bias gradient: 3->64 stride 2, 2->128 stride 1) against torch
    autograd, on maps with partial 8x8 tiles; accumulation semantics; NCHW and channel-last inputs."""
    cin, cout, k, stride, B, Ho, Wo = case
    dev = torch.device("cuda")
    tag = "bws/" + "x".join(map(str, case))
    x = gc.uni(tag + "/x", (B, cin, Ho * stride, Wo * stride), -1, 1)
    w = gc.uni(tag + "/w", (cout, cin, k, k), -0.1, 0.1).requires_grad_(True)
    b = gc.uni(tag + "/b", (cout,), -0.1, 0.1).requires_grad_(True)
    gy = gc.uni(tag + "/gy", (B, cout, Ho, Wo), -1, 1)
    y = torch.nn.functional.conv2d(x, w, b, stride=stride, padding=k // 2)
    assert y.shape[-2:] == (Ho, Wo)
    (y * gy).sum().backward()
    dy = torch.zeros(B * Ho * Wo, cout + 8, device=dev)
    dy[:, 4:4 + cout] = kc.cl(gy).to(dev)
    dw, db = torch.zeros(cout, cin, k, k, device=dev), torch.zeros(cout, device=dev)
    lib.conv2d_wgrad_small(x.to(dev), True, 0, cin, dy, 4, cout, dw, db, k, k, stride, B, Ho, Wo)
    tol = 3e-6 * float(w.grad.abs().max()) + 1e-6
    kc.check(dw, w.grad, tol, "weight gradient (NCHW input)")
    kc.check(db, b.grad, 3e-6 * float(b.grad.abs().max()) + 1e-6, "bias gradient")
    xcl = torch.full((B * Ho * stride * Wo * stride, cin + 3), 5.0, device=dev)
    xcl[:, 2:2 + cin] = kc.cl(x).to(dev)
    lib.conv2d_wgrad_small(xcl, False, 2, cin, dy, 4, cout, dw, None, k, k, stride, B, Ho, Wo)      # accumulates
    kc.check(dw, 2 * w.grad, 2 * tol, "weight gradient accumulates (channel-last input)")


# ---------------------------------------------------------------------------------------------------------------------
# Directed cases against float64 under the derived bounds of tests/wgrad_launches.py (independent of what the product launches)
# ---------------------------------------------------------------------------------------------------------------------
def _replay(lib, launch, seed, **kwargs):
    """One case: a launch, both bounds, the padding pattern and the sentinels; a second launch (without db when it has one:
    db then stays at 1x) must give 2x.  Prints the worst err / bound ratios."""
    dev = torch.device("cuda")
    case = wl.build_case(launch, launch.B, launch.H, launch.W, dev, seed=seed)
    ref = wl.reference(case)
    wl.run_case(lib, case, **kwargs)
    fails, worst = wl.check_case(case, ref, 1.0)
    db = case.T.pop("db", None)                       # second launch: dw accumulates, db is not passed
    wl.run_case(lib, case, **kwargs)
    if db is not None:
        case.T["db"] = db
    fails2, worst2 = wl.check_case(case, ref, 2.0, db_mult=1.0)
    print(f"\n{wl.sig_str(launch)}: worst err / bound dw {worst['dw'][0]:.3g} / {worst['dw'][1]:.3g} (2x: {worst2['dw'][0]:.3g} / "
          f"{worst2['dw'][1]:.3g}), db {worst['db'][0]:.3g} / {worst['db'][1]:.3g}")
    assert not fails and not fails2, "\n".join(fails + ["after the second launch:"] + fails2)


# B = 1103 (a prime) images of 3x29: every image is ONE partial tile, so consecutive tiles of a split lie in different images, and
# with the at most 512 splits pf_conv2d_wgrad's header promises every split owns two or more tiles and no split count divides 1103.
# 3 x 150x300: 380 tiles per image, partial on both edges, 1140 in all.
WG_GEOMETRIES = [(1103, 3, 29), (3, 150, 300)]
# (c0, c1, off1, cout, off_dy, pad_dy, db): single segment; [32 | 64] two segments; cout 4 and 124 at a non-zero off_dy
WG_CHANNELS = [(64, 0, 0, 64, 0, 0, True), (32, 64, 8, 124, 8, 12, False), (32, 0, 0, 4, 128, 4, True), (32, 64, 0, 124, 4, 0, True)]


@pytest.mark.parametrize("geo", WG_GEOMETRIES, ids=lambda g: "x".join(map(str, g)))
@pytest.mark.parametrize("ch", WG_CHANNELS, ids=lambda c: "c%d+%d-o%d@%d%s" % (c[0], c[1], c[3], c[4], "-db" if c[6] else ""))
@pytest.mark.parametrize("k", [(3, 3), (1, 5), (5, 1), (1, 1)], ids=lambda k: "%dx%d" % k)
def test_wgrad_splits_that_own_several_tiles(lib, k, ch, geo):
    c0, c1, off1, cout, off_dy, pad_dy, db = ch
    B, H, W = geo
    ln = wl.mfma_launch(k[0], k[1], c0, cout, B, H, W, c1=c1, off1=off1, pad0=4, pad1=8, off_dy=off_dy, pad_dy=pad_dy, db=db)
    nt, ns = wl.tiles(ln), wl.mfma_splits(ln)
    assert ns <= 512 and nt >= 2 * ns and nt % ns, (nt, ns)          # every split owns two or more tiles, unevenly
    _replay(lib, ln, seed=hash((k, ch, geo)) % 10007)


def _small_groups(lib, ln):
    """Workgroups per 64-channel column block of a pf_conv2d_wgrad_small launch, from the workspace the library asks for."""
    a = ln.args
    n = int(lib._dll.pf_conv2d_wgrad_small_ws_floats(a["cin"], a["cout"], a["kh"], a["kw"], ln.B, ln.H, ln.W))
    per = ((a["cout"] + 63) // 64) * (a["kh"] * a["kw"] * a["cin"] + 1) * 64
    assert n > 0 and n % per == 0
    return n // per


# (cin, cout, kh, kw, stride, nchw, off_in): 521 images of 7x5 outputs (one partial 8x8 tile each)
WS_CASES = [(1, 96, 7, 7, 1, False, 3), (2, 100, 7, 7, 1, False, 2), (3, 96, 7, 7, 2, True, 0), (4, 100, 7, 7, 2, False, 0),
            (1, 100, 3, 3, 2, True, 0), (2, 96, 7, 7, 2, False, 0), (3, 100, 5, 5, 1, False, 1), (4, 96, 3, 7, 1, True, 0)]


@pytest.mark.parametrize("one_stage", [False, True], ids=["ws", "one-stage"])
@pytest.mark.parametrize("case", WS_CASES, ids=lambda c: "cin%d-o%d-%dx%d-s%d-%s" % (c[0], c[1], c[2], c[3], c[4], "nchw" if c[5] else "cl%d" % c[6]))
def test_small_cin_wgrad_workgroups_that_walk_several_tiles(lib, case, one_stage):
    """Both entries on the same inputs: the two-stage pf_conv2d_wgrad_small_ws the product calls and the one-stage
    pf_conv2d_wgrad_small."""
    cin, cout, kh, kw, stride, nchw, off_in = case
    ln = wl.small_launch(cin, cout, kh, kw, stride, 521, 7, 5, nchw=nchw, off_in=off_in, pad_in=1, off_dy=4, pad_dy=8)
    groups, nt = _small_groups(lib, ln), wl.tiles(ln)
    assert nt > 2 * groups and nt % groups, (nt, groups)           # more than two tiles per workgroup, unevenly
    _replay(lib, ln, seed=hash(case) % 10007, one_stage=one_stage)


@pytest.mark.parametrize("one_stage", [False, True], ids=["ws", "one-stage"])
def test_small_cin_wgrad_with_an_empty_reduce_slice(lib, one_stage):
    """9 workgroups: the second stage's 8 slices take 2 workgroups each, so slices 5..7 are empty."""
    ln = wl.small_launch(2, 100, 7, 7, 1, 9, 7, 5, nchw=False, off_in=2, pad_in=0, off_dy=0, pad_dy=4)
    assert _small_groups(lib, ln) == 9
    _replay(lib, ln, seed=99, one_stage=one_stage)


def test_training_ops_without_pytorch_kernels(lib):
    """The autograd Functions that replaced the last PyTorch-ROCm operators of a training step against torch autograd on the
    CPU: stride-2 convolutions (zero-stuffed gradient), the 7x7 stems, frozen BatchNorm (dx, d gamma, d beta)."""
    import torch.nn as nn
    from prior_flow_amd import autograd as ag
    dev = torch.device("cuda")

    def compare(mod, x, hip_fn, tol, needs_dx=True):
        xc = x.clone().requires_grad_(needs_dx)
        ref = mod(xc)
        gy = gc.uni("tops/gy/" + type(mod).__name__ + str(tuple(ref.shape)), tuple(ref.shape), -1, 1)
        (ref * gy).sum().backward()
        want = {k: p.grad.clone() for k, p in mod.named_parameters()}
        mod.zero_grad()
        md = mod.to(dev)
        xd = x.to(dev).clone().requires_grad_(needs_dx)
        ag.STATS["hip"] = ag.STATS["torch"] = 0
        out = hip_fn(md, xd)
        kc.check(out.detach(), ref.detach(), tol * float(ref.abs().max()), "forward")
        (out * gy.to(dev)).sum().backward()
        assert ag.STATS["torch"] == 0 and ag.STATS["hip"] >= 2, ag.STATS
        for k, p in md.named_parameters():
            kc.check(p.grad, want[k], tol * float(want[k].abs().max()) + 1e-6, "d " + k)
        if needs_dx:
            kc.check(xd.grad, xc.grad, tol * float(xc.grad.abs().max()), "dx")
        mod.cpu()

    torch.manual_seed(3)
    compare(nn.Conv2d(64, 96, 3, stride=2, padding=1), gc.uni("tops/x1", (2, 64, 20, 36), -1, 1), lambda m, x: ag.conv2d(x, m), 3e-4)
    compare(nn.Conv2d(96, 128, 1, stride=2), gc.uni("tops/x2", (1, 96, 18, 10), -1, 1), lambda m, x: ag.conv2d(x, m), 3e-4)
    compare(nn.Conv2d(3, 64, 7, stride=2, padding=3), gc.uni("tops/x3", (2, 3, 40, 56), -1, 1), lambda m, x: ag.conv2d(x, m), 1e-5, needs_dx=False)
    compare(nn.Conv2d(2, 128, 7, padding=3), gc.uni("tops/x4", (1, 2, 17, 27), -3, 3), lambda m, x: ag.conv2d(x, m), 1e-5, needs_dx=False)
    bn = nn.BatchNorm2d(96)
    with torch.no_grad():
        bn.weight.copy_(gc.uni("tops/bn/w", (96,), 0.5, 1.5)); bn.bias.copy_(gc.uni("tops/bn/b", (96,), -0.3, 0.3))
        bn.running_mean.copy_(gc.uni("tops/bn/m", (96,), -0.5, 0.5)); bn.running_var.copy_(gc.uni("tops/bn/v", (96,), 0.5, 2.0))
    bn.eval()
    compare(bn, gc.uni("tops/x5", (2, 96, 12, 20), -2, 2), lambda m, x: ag._norm(m, x), 2e-5)
