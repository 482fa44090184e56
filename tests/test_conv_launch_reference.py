"""CPU checks of tests/conv_launches.py, the harness of test_hip_conv_launches.py: the launch signature and the ragged-geometry
search on the built library's host planners (fake pointers, as in test_abi.py), and proof that the float64 reference's error
bounds have teeth -- emulated wrong kernels fail them, the exact result passes with margin.  No GPU."""
import math

import pytest
import torch

import conv_launches as cl

FAKE = 0x1000            # never dereferenced: the planners only read the descriptor


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_hip()
    from prior_flow_amd import _lib
    return _lib.PfLib(_lib.LIB_PATH, require_cuda=False)


def _desc(cin, cout, kh, kw, prec=1, split=False, epi=0, **kw_):
    from prior_flow_amd import _lib
    d = _lib.ConvDesc()
    cpc = 64 if prec == 2 else 32
    if split or prec == 2:
        d.in0_split, d.lds0 = FAKE, (cin + cpc - 1) // cpc
        d.zeros, d.zeros_bytes = FAKE, 4096
    else:
        d.in0, d.ld0 = FAKE, cin
    d.c0 = cin
    d.weight = d.bias = FAKE
    d.out, d.ld_out, d.cout = FAKE, cout, cout
    d.kh, d.kw = kh, kw
    d.epilogue, d.scale, d.precision, d.stride = epi, 1.0, prec, 1
    for k, v in kw_.items():
        setattr(d, k, v)
    return d


def _launch(lib, descs, B, H, W):
    return cl.Launch(cl.signature(lib, descs, B, H, W), B, H, W, [cl._layout(d) for d in descs], "test")


# one launch per planner outcome: (descriptor arguments, geometry, tile, roles)
PLANS = [
    (dict(cin=64, cout=32, kh=3, kw=3, prec=0), (1, 64, 128), 0, 0),
    (dict(cin=64, cout=64, kh=3, kw=3, prec=0), (1, 64, 128), 1, 0),
    (dict(cin=256, cout=256, kh=3, kw=3, prec=0), (1, 64, 256), 2, 0),
    (dict(cin=128, cout=64, kh=3, kw=3), (1, 64, 128), 3, 1),
    (dict(cin=256, cout=128, kh=3, kw=3), (4, 64, 128), 4, 2),
    (dict(cin=128, cout=64, kh=3, kw=3), (16, 64, 128), 5, 0),
    (dict(cin=64, cout=64, kh=3, kw=3), (4, 256, 512), 6, 0),
    (dict(cin=64, cout=96, kh=3, kw=3, stride=2), (4, 128, 256), 7, 0),
    (dict(cin=96, cout=96, kh=3, kw=3), (4, 128, 256), 8, 0),
    (dict(cin=256, cout=128, kh=3, kw=3, split=True), (1, 64, 128), 3, 17),
    (dict(cin=256, cout=128, kh=3, kw=3, split=True), (4, 64, 128), 4, 18),
    (dict(cin=256, cout=256, kh=1, kw=5, split=True), (4, 64, 128), 4, 18),
    (dict(cin=256, cout=128, kh=3, kw=3, prec=2), (1, 64, 128), 3, 17),
]


@pytest.mark.parametrize("args,geo,tile,roles", PLANS, ids=[f"tile{p[2]}-roles{p[3]}-{cl.PREC_NAMES[p[0].get('prec', 1)]}" for p in PLANS])
def test_signature_names_the_planned_kernel(lib, args, geo, tile, roles):
    d = _desc(**args)
    sig = cl.signature(lib, [d], *geo)
    assert sig[3:5] == (f"tile{tile}", f"roles{roles}"), sig
    assert sig[0] == cl.PREC_NAMES[args.get("prec", 1)] and sig[2] == f"{args['kh']}x{args['kw']}"
    assert sig == cl.signature(lib, [_desc(**args)], *geo)          # hashable, independent of the pointer values
    hash(sig)


def test_signature_separates_forms_and_options(lib):
    base = dict(cin=256, cout=128, kh=3, kw=3)
    geo = (1, 64, 128)
    s0 = cl.signature(lib, [_desc(**base)], *geo)
    variants = [_desc(**base, out_split=FAKE, lds_out=4), _desc(**base, scale=0.25), _desc(**base, epi=1),
                _desc(**base, in_scale=FAKE, in_shift=FAKE), _desc(**base, in_scale=FAKE, in_shift=FAKE, in_relu=1),
                _desc(**base, stats_out=FAKE), _desc(**base, co_groups=1)]
    sigs = [cl.signature(lib, [d], *geo) for d in variants]
    assert len(set(sigs + [s0])) == len(sigs) + 1
    # out aliasing h (PF_EPI_ADD as train_loop launches it) is its own signature
    a = _desc(**base, epi=7, h=FAKE + 4 * 16, ld_h=256, ld_out=256, off_out=16)
    b = _desc(**base, epi=7, h=FAKE + 4096, ld_h=256, ld_out=256, off_out=16)
    sa, sb = cl.signature(lib, [a], *geo), cl.signature(lib, [b], *geo)
    assert "out=h" in sa[7][0][5] and "out=h" not in sb[7][0][5]
    # two groups, pre and save_gates
    zr = dict(cin=384, cout=256, kh=1, kw=5, split=True, epi=2, h=2 * FAKE, ld_h=128, aux_out=FAKE, ld_aux=256, ld_out=128)
    s1 = cl.signature(lib, [_desc(**zr), _desc(**zr)], *geo)
    s2 = cl.signature(lib, [_desc(**zr, save_gates=1), _desc(**zr, save_gates=1)], *geo)
    s3 = cl.signature(lib, [_desc(**zr, pre=FAKE, ld_pre=256), _desc(**zr, pre=FAKE, ld_pre=256)], *geo)
    assert s1[5] == "groups2" and len({s1, s2, s3}) == 3


def test_f16_launches_outside_the_dma_kernel_are_refused(lib):
    """PF_PREC_F16 exists on the all-DMA kernel only: a 1x1, a stride-2 or a fused-statistics f16 launch is an error."""
    from prior_flow_amd import _lib
    geo = (1, 64, 128)
    for bad in (_desc(256, 128, 1, 1, prec=2), _desc(256, 128, 3, 3, prec=2, stride=2), _desc(256, 128, 3, 3, prec=2, stats_out=FAKE),
                _desc(256, 128, 3, 3, prec=2, in_scale=FAKE, in_shift=FAKE)):
        assert cl.plan(lib, [bad], *geo)[0] < 0
    ok = _desc(256, 128, 3, 3, prec=2)
    assert cl.plan(lib, [ok], *geo) == (3, 17)
    fp32_operand = _desc(256, 128, 3, 3, prec=2)
    fp32_operand.in0, fp32_operand.ld0, fp32_operand.in0_split = FAKE, 256, None
    arr = (_lib.ConvDesc * 1)(fp32_operand)
    assert lib._dll.pf_conv2d_tile(arr, 1, *geo) < 0


@pytest.mark.parametrize("args,geo,tile,roles", [p for p in PLANS if p[2] != 6], ids=[f"tile{p[2]}-roles{p[3]}" for p in PLANS if p[2] != 6])
def test_ragged_sibling_keeps_the_signature(lib, args, geo, tile, roles):
    launch = _launch(lib, [_desc(**args)], *geo)
    sib = cl.ragged_sibling(lib, launch)
    assert sib is not None, cl.why_no_sibling(lib, launch)
    B, H, W = sib
    assert B >= 2 and H % 8 and W % 32 and (B * H * W) % 64
    assert cl.signature(lib, [_desc(**args)], B, H, W) == launch.sig


def test_tile6_has_no_ragged_sibling_and_says_why(lib):
    launch = _launch(lib, [_desc(64, 64, 3, 3)], 4, 256, 512)
    assert launch.sig[3] == "tile6"
    assert cl.ragged_sibling(lib, launch) is None
    assert "32-column" in cl.why_no_sibling(lib, launch)


# ---------------------------------------------------------------------------------------------------------------------
# the bounds have teeth
# ---------------------------------------------------------------------------------------------------------------------
def _split(t):
    hi = t.float().to(torch.bfloat16).double()
    lo = (t.float() - hi.float()).to(torch.bfloat16).double()
    return hi, lo


def _emulated(kind):
    """conv_fp64 replacements that compute what a (wrong) kernel would: from .bfloat16() operands in float64."""
    def conv(x, w, B, H, W, stride):
        exact = cl.conv_fp64(x, w, B, H, W, stride)
        if kind == "exact":
            return exact
        xh, xl = _split(x)
        wh, wl = _split(w)
        f = lambda a, b: cl.conv_fp64(a, b, B, H, W, stride, terms=("acc",))["acc"]     # noqa: E731
        if kind == "bf16x3":
            acc = f(xh, wh) + f(xh, wl) + f(xl, wh)
        elif kind == "no_hi_lo":
            acc = f(xh, wh) + f(xl, wh)
        elif kind == "bf16x1":
            acc = f(xh, wh)
        elif kind == "unrounded":        # fp16 conv computed from the fp32 operands instead of the fp16-rounded ones
            return exact
        elif kind == "border_tap":       # left border: the kx = 0 tap reads the previous row's last pixel instead of zero padding
            cin = x.shape[1]
            xi = x.reshape(B, H, W, cin)
            wrap = torch.zeros_like(xi)
            wrap[:, 1:, 0, :] = xi[:, :-1, W - 1, :]
            # contribution of the padding column as seen by output column 0 through tap kx = 0
            kh, kw = w.shape[2], w.shape[3]
            extra = torch.zeros(B, H, W, w.shape[0], dtype=torch.float64)
            wpad = torch.nn.functional.pad(wrap[:, :, 0, :], (0, 0, kh // 2, kh - 1 - kh // 2))
            for ky in range(kh):
                extra[:, :, 0, :] += wpad[:, ky:ky + H, :].double() @ w[:, :, ky, 0].double().t()
            acc = exact["acc"] + extra.reshape(-1, w.shape[0])
        out = dict(exact)
        out["acc"] = acc
        return out
    return conv


def _teeth_case(lib, prec, cin, cout, kh, kw, B=2, H=9, W=37, epi=0, scale=1.0, **extra):
    d = _desc(cin, cout, kh, kw, prec=prec, split=(prec == 2), epi=epi, scale=scale, **extra)
    launch = _launch(lib, [d], B, H, W)
    return cl.build_case(lib, launch, B, H, W, torch.device("cpu"), seed=11)


def _run(case, kind):
    """(per-element failures, aggregate failures, worst aggregate ratio) of an emulated kernel against the float64 reference."""
    ref = cl.reference(case)[0]["out"]
    got = cl.reference(case, conv=_emulated(kind))[0]["out"]["ref"]
    if kind == "unrounded":                       # the same launch with the operands left in fp32
        g = case.groups[0]
        saved = g["precision"]
        g["precision"] = 1
        got = cl.reference(case)[0]["out"]["ref"]
        g["precision"] = saved
    fails = []
    _, agg = cl.compare(got, ref, kind, fails)
    return [f for f in fails if "per-element" in f], [f for f in fails if "aggregate" in f], agg


BF16X3_TYPICAL = [(256, 128, 3, 3), (384, 256, 1, 5), (64, 64, 3, 3)]


@pytest.mark.parametrize("cin,cout,kh,kw", BF16X3_TYPICAL)
def test_bf16x3_bounds_have_teeth(lib, cin, cout, kh, kw):
    case = _teeth_case(lib, 1, cin, cout, kh, kw)
    e, a, agg = _run(case, "exact")
    assert not e and not a and agg == 0.0
    e, a, agg = _run(case, "bf16x3")                 # the arithmetic the header specifies passes with margin
    assert not e and not a and agg <= 0.25, agg
    for kind in ("no_hi_lo", "bf16x1"):               # ~40x and ~60x the aggregate bound
        e, a, agg = _run(case, kind)
        assert a, f"{kind}: aggregate check did not fail (err / bound = {agg:.3g})"
        assert agg > 10, agg


@pytest.mark.parametrize("cin,cout,kh,kw", [(256, 128, 3, 3), (384, 256, 1, 5), (384, 128, 5, 1)])
def test_f16_bound_refuses_unrounded_operands(lib, cin, cout, kh, kw):
    case = _teeth_case(lib, 2, cin, cout, kh, kw)
    e, a, agg = _run(case, "exact")
    assert not e and not a
    e, a, agg = _run(case, "unrounded")                # ~30x the aggregate bound
    assert a and agg > 10, f"fp32 operands passed the fp16 bound (err / bound = {agg:.3g})"


@pytest.mark.parametrize("prec", [0, 1, 2])
@pytest.mark.parametrize("cin,cout,kh,kw", [(128, 64, 3, 3), (256, 128, 1, 5)])
def test_border_tap_shift_fails_per_element(lib, prec, cin, cout, kh, kw):
    case = _teeth_case(lib, prec, cin, cout, kh, kw)
    e, a, _ = _run(case, "border_tap")
    assert e, "a one-tap shift at the left border passed the per-element check"


@pytest.mark.parametrize("epi", [2, 3, 4, 6, 7])
def test_epilogue_bounds_pass_the_exact_result_and_refuse_a_wrong_epilogue(lib, epi):
    """The bounds carried through the epilogues: the exact fp64 result passes; the same data through a different epilogue
    (or without its bias or its scale) does not."""
    cout = {2: 256, 3: 128, 4: 256, 6: 128, 7: 128}[epi]
    kw_ = dict(h=2 * FAKE, ld_h=256, ld_out=256)
    if epi == 2:
        kw_.update(aux_out=FAKE, ld_aux=256, save_gates=1)
    if epi == 3:
        kw_.update(z=FAKE, ld_z=128, aux_out=FAKE, ld_aux=128, save_gates=1)
    if epi == 4:
        kw_ = dict(aux_out=FAKE, ld_aux=128, ld_out=128)
    case = _teeth_case(lib, 1, 256, cout, 1, 5, epi=epi, scale=0.25 if epi in (6, 7) else 1.0, **kw_)
    refs = cl.reference(case)[0]
    for name, r in refs.items():
        fails = []
        cl.compare(r["ref"], r, name, fails)
        assert not fails
    g = case.groups[0]
    b = g["T"]["b"].clone()
    g["T"]["b"].zero_()                                # the kernel that drops the bias
    wrong = cl.reference(case)[0]
    g["T"]["b"].copy_(b)
    fails = []
    cl.compare(wrong["out"]["ref"], refs["out"], "no bias", fails)
    assert fails
    if epi in (6, 7):
        g["scale"] = 1.0                               # the kernel that ignores `scale`
        wrong = cl.reference(case)[0]
        g["scale"] = 0.25
        fails = []
        cl.compare(wrong["out"]["ref"], refs["out"], "no scale", fails)
        assert fails
    if epi == 6:                                       # the mask input has exact +0.0 and -0.0 and both signs
        h = g["T"]["h_val"]
        assert bool((h == 0).any()) and bool(torch.signbit(h[h == 0]).any()) and bool((~torch.signbit(h[h == 0])).any())
        assert 0.4 < float((h <= 0).double().mean()) < 0.6


def test_reference_is_float64_conv2d():
    """conv_fp64 (per-tap float64 matmuls, both strides, odd and even kernels) == torch's float64 conv2d on the CPU."""
    g = torch.Generator().manual_seed(3)
    for (kh, kw, s) in ((3, 3, 1), (1, 5, 1), (5, 1, 1), (3, 3, 2), (1, 1, 2), (4, 4, 1), (7, 7, 1)):
        B, H, W, cin, cout = 2, 7, 11, 12, 5
        x = torch.randn(B * H * s * W * s, cin, generator=g, dtype=torch.float64)
        w = torch.randn(cout, cin, kh, kw, generator=g, dtype=torch.float64)
        got = cl.conv_fp64(x, w, B, H, W, s, max_elems=4000)
        xn = x.view(B, H * s, W * s, cin).permute(0, 3, 1, 2)
        xn = torch.nn.functional.pad(xn, (kw // 2, kw - 1 - kw // 2, kh // 2, kh - 1 - kh // 2))
        want = torch.nn.functional.conv2d(xn, w, stride=s)[:, :, :H, :W].permute(0, 2, 3, 1).reshape(-1, cout)
        assert torch.allclose(got["acc"], want, rtol=1e-12, atol=1e-12), (kh, kw, s)
        absw = torch.nn.functional.conv2d(xn.abs(), w.abs(), stride=s)[:, :, :H, :W].permute(0, 2, 3, 1).reshape(-1, cout)
        assert torch.allclose(got["abs"], absw, rtol=1e-12, atol=1e-12)
        assert math.isclose(float(got["sq"].sum()), float(torch.nn.functional.conv2d(xn * xn, w * w, stride=s)[:, :, :H, :W].sum()), rel_tol=1e-12)
