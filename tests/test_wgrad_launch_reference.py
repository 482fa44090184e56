"""CPU checks of tests/wgrad_launches.py, the harness of test_hip_wgrad_launches.py and of the directed cases in
test_hip_conv_bwd.py: the float64 reference against torch's own float64 weight gradient, the case builder's layout, proof that
the two error bounds have teeth -- an emulation of the MFMA kernel's arithmetic passes them with margin, five wrong kernels
fail the AGGREGATE one -- and the argument checks of pf_conv2d_wgrad / pf_conv2d_wgrad_small[_ws] on the built library (fake
pointers, as in test_abi.py: they all return before any launch).  No GPU."""
import pytest
import torch

import wgrad_launches as wl
from conv_launches import SENT_IN

FAKE = 0x10000           # never dereferenced: every call below is refused before a launch
BAD_ARG, BAD_SHAPE = -1, -2


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_hip()
    from prior_flow_amd import _lib
    return _lib.PfLib(_lib.LIB_PATH, require_cuda=False)


# ---------------------------------------------------------------------------------------------------------------------
# reference and case builder
# ---------------------------------------------------------------------------------------------------------------------
def test_reference_is_float64_autograd():
    """wgrad_fp64 (per-tap float64 matmuls, chunked by images) == the weight gradient torch's float64 autograd gives."""
    g = torch.Generator().manual_seed(4)
    for kh, kw, s in ((3, 3, 1), (1, 5, 1), (5, 1, 1), (1, 1, 1), (7, 7, 1), (7, 7, 2), (3, 3, 2)):
        B, H, W, cin, cout = 3, 7, 11, 5, 6
        x = torch.randn(B, cin, H * s, W * s, generator=g, dtype=torch.float64)
        w = torch.zeros(cout, cin, kh, kw, dtype=torch.float64, requires_grad=True)
        gy = torch.randn(B, cout, H, W, generator=g, dtype=torch.float64)
        y = torch.nn.functional.conv2d(x, w, stride=s, padding=(kh // 2, kw // 2))
        assert y.shape == gy.shape
        (y * gy).sum().backward()
        xr = x.permute(0, 2, 3, 1).reshape(-1, cin)
        dyr = gy.permute(0, 2, 3, 1).reshape(-1, cout)
        got = wl.wgrad_fp64(xr, dyr, B, H, W, kh, kw, s, max_elems=3000)
        want = w.grad.permute(0, 2, 3, 1).reshape(cout, kh * kw, cin)
        assert torch.allclose(got["acc"], want, rtol=1e-12, atol=1e-12), (kh, kw, s)
        one = wl.wgrad_fp64(xr.abs(), dyr.abs(), B, H, W, kh, kw, s, terms=("acc",))["acc"]
        assert torch.allclose(got["abs"], one, rtol=1e-12, atol=1e-12)
        sq = wl.wgrad_fp64(xr * xr, dyr * dyr, B, H, W, kh, kw, s, terms=("acc",))["acc"]
        assert torch.allclose(got["sq"], sq, rtol=1e-12, atol=1e-12)


def test_build_case_layout_and_checks():
    """Sentinels outside the read slices, zeros in the live region, a non-zero pattern in the padding; check_case passes the
    exact result and refuses a write into the padding, a wrong db and a value off by one tile."""
    dev = torch.device("cpu")
    ln = wl.mfma_launch(3, 3, 32, 124, 2, 9, 37, c1=40, off0=4, off1=8, off_dy=12, pad0=4, pad1=4, pad_dy=8, dw_rows=256)
    assert ln.args["dw_shape"] == (256, 9, 96) and ln.sig == wl.mfma_launch(3, 3, 32, 124, 2, 9, 37, c1=40, off0=4, off1=8, off_dy=12,
                                                                             pad0=4, pad1=4, pad_dy=8, dw_rows=256).sig
    hash(ln.sig)
    case = wl.build_case(ln, 2, 9, 37, dev, seed=3)
    T = case.T
    assert T["x0"].shape == (666, 40) and T["x1"].shape == (666, 52) and T["dy"].shape == (666, 144)
    assert bool((T["x0"][:, :4] == SENT_IN).all()) and bool((T["x0"][:, 36:] == SENT_IN).all())
    assert bool((T["dy"][:, :12] == SENT_IN).all()) and bool((T["dy"][:, 136:] == SENT_IN).all())
    assert float(T["dw"][:124, :, :72].abs().max()) == 0 and float(T["db"][:124].abs().max()) == 0
    assert bool((T["dw"][124:] != 0).all()) and bool((T["dw"][:, :, 72:] != 0).all()) and bool((T["db"][124:] != 0).all())
    ref = wl.reference(case)
    assert ref["K"] == 666 and ref["dw"]["ref"].shape == (124, 9, 72)
    T["dw"][:124, :, :72] = ref["dw"]["ref"].float()
    T["db"][:124] = ref["db"]["ref"].float()
    fails, worst = wl.check_case(case, ref)
    assert not fails and worst["dw"][1] < 0.1, fails
    T["dw"][130, 2, 5] = 0.0
    assert any("padding" in f for f in wl.check_case(case, ref)[0])
    T["dw"].copy_(T["dw_init"])
    T["dw"][:124, :, :72] = ref["dw"]["ref"].float()
    T["db"][3] += 1e-3
    assert any(f.startswith("db") for f in wl.check_case(case, ref)[0])
    T["db"][3] -= 1e-3
    T["dy"][5, 140] = 0.0
    assert any("dy" in f for f in wl.check_case(case, ref)[0])
    # the small kernel's layout: [Cout][Cin][KH][KW], stride 2, NCHW planes and a channel-last slice
    for nchw in (True, False):
        ls = wl.small_launch(3, 8, 7, 7, 2, 2, 5, 6, nchw=nchw, off_in=2, pad_in=3, off_dy=4, pad_dy=4)
        cs = wl.build_case(ls, 2, 5, 6, dev, seed=4)
        assert cs.T["x"].shape == ((2, 3, 10, 12) if nchw else (240, 8)) and cs.T["dw"].shape == (8, 3, 7, 7)
        x = cs.T["x_val"].double().view(2, 10, 12, 3).permute(0, 3, 1, 2)
        w = torch.zeros(8, 3, 7, 7, dtype=torch.float64, requires_grad=True)
        gy = cs.T["dy_val"].double().view(2, 5, 6, 8).permute(0, 3, 1, 2)
        (torch.nn.functional.conv2d(x, w, stride=2, padding=3) * gy).sum().backward()
        assert torch.allclose(wl.reference(cs)["dw"]["ref"], w.grad, rtol=1e-12, atol=1e-12)


def test_recorder_records_layout_and_restores(monkeypatch):
    """The recorder on stubbed entries (nothing is launched): leading dimensions, offsets, dw.shape, db / x1 presence and the
    geometry make the signature; equal launches share it; the class is restored on exit."""
    from prior_flow_amd import _lib
    calls = []
    monkeypatch.setattr(_lib.PfLib, "conv2d_wgrad", lambda self, *a, **k: calls.append(("mfma", a, k)))
    monkeypatch.setattr(_lib.PfLib, "conv2d_wgrad_small", lambda self, *a, **k: calls.append(("small", a, k)))
    stub_m, stub_s = _lib.PfLib.conv2d_wgrad, _lib.PfLib.conv2d_wgrad_small
    lib = object.__new__(_lib.PfLib)
    x0, x1, dy = torch.zeros(24, 40), torch.zeros(24, 72), torch.zeros(24, 272)
    dw, db = torch.zeros(128, 5, 96), torch.zeros(128)
    with wl.Recorder("p") as rec:
        lib.conv2d_wgrad(x0, 4, 32, dy, 192, 64, dw, db, 1, 5, 2, 3, 4, x1=x1, off1=8, c1=64)
        lib.conv2d_wgrad(x0, 4, 32, dy, 192, 64, dw, db, 1, 5, 2, 3, 4, x1=x1, off1=8, c1=64)
        lib.conv2d_wgrad(x0, 4, 32, dy, 192, 64, dw[:, :, :32], None, 1, 5, 2, 3, 4)
        lib.conv2d_wgrad_small(torch.zeros(24, 4), False, 2, 2, dy, 0, 128, torch.zeros(128, 2, 7, 7), db, 7, 7, 1, 2, 3, 4)
        lib.conv2d_wgrad_small(torch.zeros(2, 3, 6, 8), True, 0, 3, dy, 0, 64, torch.zeros(64, 3, 7, 7), None, 7, 7, 2, 2, 3, 4, one_stage=True)
    assert _lib.PfLib.conv2d_wgrad is stub_m and _lib.PfLib.conv2d_wgrad_small is stub_s
    assert [c[0] for c in calls] == ["mfma", "mfma", "mfma", "small", "small"] and calls[4][2] == {"one_stage": True}
    a, b, c, d, e = rec.launches
    assert a.sig == b.sig != c.sig and len({l.sig for l in rec.launches}) == 4 and a.path == "p"
    assert a.args == dict(ld0=40, off0=4, c0=32, ld1=72, off1=8, c1=64, ld_dy=272, off_dy=192, cout=64, kh=1, kw=5,
                          dw_shape=(128, 5, 96), db_len=128, has_x1=True) and (a.B, a.H, a.W) == (2, 3, 4)
    assert c.args["dw_shape"] == (128, 5, 32) and c.args["db_len"] == 0 and not c.args["has_x1"]
    assert d.args["ld_in"] == 4 and d.args["off_in"] == 2 and not d.args["nchw"] and d.args["dw_shape"] == (128, 2, 7, 7)
    assert e.args["nchw"] and e.args["ld_in"] == 0 and e.args["stride"] == 2 and e.args["db_len"] == 0
    case = wl.build_case(a, 2, 3, 4, torch.device("cpu"))               # a recorded launch builds like a hand-written one
    assert case.T["x1"].shape == (24, 72) and case.T["dy"].shape == (24, 272) and case.T["dw"].shape == (128, 5, 96)


def test_geometry_helpers():
    ln = wl.mfma_launch(1, 1, 256, 576, 12, 48, 64)
    assert wl.tiles(ln) == 288 and wl.mfma_splits(ln) == 26 and wl.ragged_sibling(ln) == (12, 47, 61)
    assert wl.mfma_splits(wl.mfma_launch(3, 3, 64, 64, 4, 192, 256)) == 256
    assert wl.ragged_sibling(wl.mfma_launch(3, 3, 64, 64, 1, 17, 27)) is None          # 16 rows are one tile row less
    assert wl.mfma_splits(wl.mfma_launch(3, 3, 64, 64, 2, 8, 32)) == 4                  # never more splits than tiles
    ls = wl.small_launch(2, 128, 7, 7, 1, 12, 48, 64)
    assert wl.tiles(ls) == 576 and wl.ragged_sibling(ls) == (12, 47, 61)


# ---------------------------------------------------------------------------------------------------------------------
# the bounds have teeth: an emulation of pf_wgrad_kernel's arithmetic and five wrong kernels
# ---------------------------------------------------------------------------------------------------------------------
def _split(t):
    hi = t.float().to(torch.bfloat16)
    lo = (t.float() - hi.float()).to(torch.bfloat16)
    return hi.float(), lo.float()                 # bf16 values, held in fp32 (exact)


def _tile_order(t, B, H, W):
    """[B*H*W, C] -> [tiles, 8 K-steps, 16 px, C]: 4 x 32 tiles (H % 4 == 0, W % 32 == 0), K-step ks = row ks / 2, half ks % 2."""
    C = t.shape[1]
    return t.view(B, H // 4, 4, W // 32, 32, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, 8, 16, C)


def _shifted(x, B, H, W, dy_, dx_, wrap_images=False):
    """x[p + (dy_, dx_)] per pixel p, zero outside the image; wrap_images: rows above / below an image come from the
    neighbouring image of the flat [B*H*W] array (a halo without the image-boundary test), zero before the first / after the last."""
    C, P = x.shape[1], 2
    if wrap_images:
        flat = torch.nn.functional.pad(x.view(B * H, W, C), (0, 0, P, P, P, P))
        return flat[P + dy_:P + dy_ + B * H, P + dx_:P + dx_ + W].reshape(B * H * W, C)
    xp = torch.nn.functional.pad(x.view(B, H, W, C), (0, 0, P, P, P, P))
    return xp[:, P + dy_:P + dy_ + H, P + dx_:P + dx_ + W].reshape(B * H * W, C)


class Emu:
    """pf_wgrad_kernel<3,3> for one 32 x 32 channel block: operands as bf16 hi / lo, per 16-pixel K-step and pass an exact
    dot (float64 holds the 16 products of 16-bit significands exactly) added to an fp32 accumulator, the passes in the kernel's
    order (lo*hi, hi*lo, hi*hi), the tiles split, split + nsplit, ... per split, then the splits added in fp32."""

    def __init__(self, x, dy, B, H, W, nsplit):
        self.x, self.B, self.H, self.W, self.ns = x, B, H, W, nsplit
        self.ntiles = B * (H // 4) * (W // 32)
        self.dyh, self.dyl = (_tile_order(t, B, H, W) for t in _split(dy))
        self.taps = [(ky - 1, kx - 1) for ky in range(3) for kx in range(3)]

    def schedule(self):
        rounds = (self.ntiles + self.ns - 1) // self.ns
        t = torch.arange(rounds)[:, None] * self.ns + torch.arange(self.ns)[None, :]
        return torch.where(t < self.ntiles, t, torch.full_like(t, -1))               # [rounds, nsplit], -1 = none

    def operand(self, taps, shift=(0, 0), wrap_images=False):
        hs, ls = [], []
        for (a, b) in taps:
            h, l = _split(_shifted(self.x, self.B, self.H, self.W, a + shift[0], b + shift[1], wrap_images))
            hs.append(_tile_order(h, self.B, self.H, self.W))
            ls.append(_tile_order(l, self.B, self.H, self.W))
        return torch.stack(hs), torch.stack(ls)                                       # [taps, tiles, 8, 16, 32]

    def partials(self, xh, xl, sched, hi_lo=True):
        """fp32 accumulators [splits, taps, 32 out, 32 in] of the splits whose tile lists are the columns of sched."""
        nt, ns = xh.shape[0], sched.shape[1]
        acc = torch.zeros(ns, nt, 32, 32, dtype=torch.float32)
        for r in range(sched.shape[0]):
            idx = sched[r].clamp_min(0)
            live = (sched[r] >= 0).double().view(ns, 1, 1, 1)
            for ks in range(8):
                ah = self.dyh[idx, ks].double().transpose(1, 2)[:, None]                       # [ns, 1, 32, 16]
                al = self.dyl[idx, ks].double().transpose(1, 2)[:, None]
                bh = xh[:, idx, ks].double().transpose(0, 1)                                    # [ns, taps, 16, 32]
                bl = xl[:, idx, ks].double().transpose(0, 1)
                for a_, b_ in ((al, bh), (ah, bl), (ah, bh)) if hi_lo else ((al, bh), (ah, bh)):
                    acc = (acc.double() + live * torch.matmul(a_, b_)).float()
        return acc

    @staticmethod
    def total(part):
        out = torch.zeros_like(part[0])
        for s in range(part.shape[0]):                                                # one fp32 atomic per split
            out = out + part[s]
        return out.transpose(0, 1).contiguous()                                       # [32 out, taps, 32 in] like dw


TEETH = [  # B, H, W, nsplit, fraction of dy kept
    pytest.param(12, 48, 64, 64, 1, id="K36864"),            # the loop's deferred gradients: 288 tiles, 4.5 per split
    pytest.param(4, 192, 256, 256, 4, id="K196608-dy-quarter"),   # an encoder's zero-stuffed stride-2 gradient: 1536 tiles over 256 splits
]


@pytest.mark.parametrize("B,H,W,nsplit,stuff", TEETH)
def test_mfma_bounds_have_teeth(B, H, W, nsplit, stuff):
    K = B * H * W
    ln = wl.mfma_launch(3, 3, 32, 32, B, H, W)
    keep = None
    if stuff > 1:                                     # dy != 0 at even rows and columns only
        keep = torch.zeros(B, H, W)
        keep[:, ::2, ::2] = 1
    case = wl.build_case(ln, B, H, W, torch.device("cpu"), seed=17, dy_keep=keep)
    ref = wl.reference(case)
    x, dy = case.T["x_val"], case.T["dy_val"]
    emu = Emu(x, dy, B, H, W, nsplit)
    sched = emu.schedule()
    assert sched.shape[0] >= 5 and int((sched >= 0).sum()) == emu.ntiles == K // 128

    def run(got):
        fails = []
        e, a = wl.compare(got, ref["dw"], K, "dw", fails)
        return e, a, [f for f in fails if "per-element" in f], [f for f in fails if "aggregate" in f]

    xh, xl = emu.operand(emu.taps)
    part = emu.partials(xh, xl, sched)
    e, a, fe, fa = run(Emu.total(part))
    print(f"\nK = {K}: faithful emulation: per-element {e:.3g}, aggregate {a:.3g} of the bound")
    assert not fe and not fa and a <= 0.25, (e, a)
    # the exact result and its fp32 rounding pass trivially
    assert run(ref["dw"]["ref"].float())[1] < 0.01

    variants = {}
    variants["hi*lo pass lost"] = Emu.total(emu.partials(xh, xl, sched, hi_lo=False))
    s, r = 5, 1                                        # split 5's second tile
    lost = sched[:, s:s + 1].clone()
    lost[r] = -1
    p = part.clone()
    p[s] = emu.partials(xh, xl, lost)[0]
    variants["one 4x32 tile lost"] = Emu.total(p)
    twice = torch.cat([sched[:, s:s + 1], sched[r:r + 1, s:s + 1]])
    p = part.clone()
    p[s] = emu.partials(xh, xl, twice)[0]
    variants["one tile added twice"] = Emu.total(p)
    t = 5                                              # tap (ky, kx) = (1, 2) reads one pixel further right
    sh, sl = emu.operand([emu.taps[t]], shift=(0, 1))
    p = part.clone()
    p[:, t] = emu.partials(sh, sl, sched)[:, 0]
    variants["a tap shifted by one pixel"] = Emu.total(p)
    rows = [i for i, (a_, _) in enumerate(emu.taps) if a_ != 0]
    wh, wl_ = emu.operand([emu.taps[i] for i in rows], wrap_images=True)
    p = part.clone()
    p[:, rows] = emu.partials(wh, wl_, sched)
    variants["a halo that reads the neighbouring image"] = Emu.total(p)
    for name, got in variants.items():
        e, a, fe, fa = run(got)
        print(f"K = {K}: {name}: per-element {e:.3g}, aggregate {a:.3g} of the bound")
        assert fa and a > 4, f"{name}: the aggregate bound did not fail (err / bound = {a:.3g})"


def test_small_and_bias_bounds_have_teeth():
    """The fp32-rounded exact dw and torch's fp32 sum for db pass; a lost 8x8 tile fails the aggregate bound of both."""
    B, H, W = 12, 48, 64
    K = B * H * W
    ln = wl.small_launch(2, 8, 7, 7, 1, B, H, W, nchw=False)
    case = wl.build_case(ln, B, H, W, torch.device("cpu"), seed=5)
    ref = wl.reference(case)
    x, dy = case.T["x_val"], case.T["dy_val"]
    got = wl.wgrad_fp64(x.float(), dy.float(), B, H, W, 7, 7, 1, terms=("acc",), max_elems=1 << 22)["acc"]     # chunks summed in fp64 ...
    got = got.permute(0, 2, 1).reshape(8, 2, 7, 7).float()                                                        # ... then one rounding
    fails = []
    wl.compare(got, ref["dw"], K, "dw", fails)
    wl.compare(dy.sum(0), ref["db"], K, "db", fails)                  # torch's fp32 sum
    assert not fails, fails
    dy2 = dy.clone().view(B, H, W, -1)
    dy2[7, 8:16, 24:32] = 0                                           # one 8x8 tile never visited
    dy2 = dy2.view(K, -1)
    lost = wl.wgrad_fp64(x, dy2, B, H, W, 7, 7, 1, terms=("acc",))["acc"].permute(0, 2, 1).reshape(8, 2, 7, 7)
    for name, g, r in (("dw", lost, ref["dw"]), ("db", dy2.double().sum(0), ref["db"])):
        fails = []
        _, a = wl.compare(g, r, K, name, fails)
        assert any("aggregate" in f for f in fails) and a > 10, (name, a)


# ---------------------------------------------------------------------------------------------------------------------
# refusals: every one returns before any launch
# ---------------------------------------------------------------------------------------------------------------------
def _wgrad(lib, **kw):
    a = dict(x0=FAKE, ld0=64, off0=0, c0=64, x1=None, ld1=0, off1=0, c1=0, dy=2 * FAKE, ld_dy=128, off_dy=0, cout=128, dw=3 * FAKE,
             db=4 * FAKE, kh=3, kw=3, B=1, H=8, W=32)
    a.update(kw)
    return lib._dll.pf_conv2d_wgrad(a["x0"], a["ld0"], a["off0"], a["c0"], a["x1"], a["ld1"], a["off1"], a["c1"], a["dy"], a["ld_dy"],
                                    a["off_dy"], a["cout"], a["dw"], a["db"], a["kh"], a["kw"], a["B"], a["H"], a["W"], None)


def test_pf_conv2d_wgrad_refusals(lib):
    for k in ((2, 2), (7, 7), (3, 1), (1, 3), (5, 5), (3, 5)):                      # a kernel shape outside the four
        assert _wgrad(lib, kh=k[0], kw=k[1]) == BAD_SHAPE, k
    for bad in (dict(cout=126), dict(c0=62, ld0=64), dict(ld0=66), dict(ld_dy=130), dict(off0=2, ld0=68), dict(off_dy=2, ld_dy=132),
                dict(x1=FAKE, c1=30, ld1=32), dict(x1=FAKE, c1=32, ld1=34), dict(x1=FAKE, c1=32, ld1=36, off1=2)):
        assert _wgrad(lib, **bad) == BAD_SHAPE, bad                                  # cout, c, ld or an offset not a multiple of 4
    assert _wgrad(lib, c0=48, ld0=48, x1=FAKE, c1=32, ld1=32) == BAD_SHAPE           # c1 > 0 with c0 % 32 != 0
    for bad in (dict(off0=4), dict(off_dy=4), dict(x1=FAKE, c1=32, ld1=32, off1=4), dict(off0=-4), dict(off_dy=-4)):
        assert _wgrad(lib, **bad) == BAD_ARG, bad                                    # a slice past (or before) its row
    for bad in (dict(x0=None), dict(dy=None), dict(dw=None), dict(c1=32, ld1=32)):  # a null operand (x1 with c1 > 0)
        assert _wgrad(lib, **bad) == BAD_ARG, bad
    for bad in (dict(B=0), dict(H=0), dict(W=0), dict(c0=0), dict(cout=0), dict(c1=-4)):
        assert _wgrad(lib, **bad) == BAD_SHAPE, bad


def _small(lib, entry="pf_conv2d_wgrad_small", ws=None, ws_floats=0, **kw):
    a = dict(x=FAKE, nchw=0, ld_in=4, off_in=0, cin=2, dy=2 * FAKE, ld_dy=128, off_dy=0, cout=128, dw=3 * FAKE, db=4 * FAKE, kh=7, kw=7,
             stride=1, B=1, H=8, W=8)
    a.update(kw)
    args = [a["x"], a["nchw"], a["ld_in"], a["off_in"], a["cin"], a["dy"], a["ld_dy"], a["off_dy"], a["cout"], a["dw"], a["db"],
            a["kh"], a["kw"], a["stride"], a["B"], a["H"], a["W"]]
    if entry.endswith("_ws"):
        return getattr(lib._dll, entry)(*args, ws, ws_floats, None)
    return getattr(lib._dll, entry)(*args, None)


def test_pf_conv2d_wgrad_small_refusals(lib):
    need = int(lib._dll.pf_conv2d_wgrad_small_ws_floats(2, 128, 7, 7, 1, 8, 8))
    assert need == 1 * 2 * (49 * 2 + 1) * 64
    for entry, extra in (("pf_conv2d_wgrad_small", {}), ("pf_conv2d_wgrad_small_ws", dict(ws=5 * FAKE, ws_floats=1 << 30))):
        assert _small(lib, entry, cin=5, ld_in=8, **extra) == BAD_SHAPE              # cin > 4
        assert _small(lib, entry, stride=3, **extra) == BAD_SHAPE
        assert _small(lib, entry, stride=0, **extra) == BAD_SHAPE
        assert _small(lib, entry, kh=7, kw=8, **extra) == BAD_SHAPE                  # kh * kw > 52
        assert _small(lib, entry, kh=53, kw=1, **extra) == BAD_SHAPE
        assert _small(lib, entry, cout=126, **extra) == BAD_SHAPE
        assert _small(lib, entry, off_dy=2, **extra) == BAD_SHAPE
        assert _small(lib, entry, off_dy=4, **extra) == BAD_ARG                      # dy slice past its row
        assert _small(lib, entry, off_in=3, **extra) == BAD_ARG                      # x slice past its row
        for ptr in ("x", "dy", "dw"):
            assert _small(lib, entry, **{ptr: None}, **extra) == BAD_ARG, ptr
    # the workspace form: a null or short workspace
    assert _small(lib, "pf_conv2d_wgrad_small_ws", ws=None, ws_floats=need) == BAD_ARG
    assert _small(lib, "pf_conv2d_wgrad_small_ws", ws=5 * FAKE, ws_floats=need - 1) == BAD_ARG
    assert _small(lib, "pf_conv2d_wgrad_small_ws", ws=5 * FAKE, ws_floats=0) == BAD_ARG
    assert int(lib._dll.pf_conv2d_wgrad_small_ws_floats(2, 128, 7, 7, 0, 8, 8)) == 0
