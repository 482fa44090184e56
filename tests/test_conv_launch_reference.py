"""CPU checks of tests/conv_launches.py, the harness of test_hip_conv_launches.py: the launch signature and the ragged-geometry
search and the enumeration of reachable plans on the built library's host planners (fake pointers, as in test_abi.py), and proof that the float64 reference's error
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


def _launch(lib, descs, B, H, W, image=None):
    return cl.Launch(cl.signature(lib, descs, B, H, W), B, H, W, [cl._layout(d) for d in descs], "test", image)


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
# the plans a layout reaches over the supported geometries
# ---------------------------------------------------------------------------------------------------------------------
def _f16_zr():
    """The f16 GRU z|r convolution as the update block launches it: 1x5, 256 -> 256, two groups, r*h into an f16 map."""
    zr = dict(cin=256, cout=256, kh=1, kw=5, prec=2, epi=2, h=2 * FAKE, ld_h=128, ld_out=128, aux_split=FAKE, lds_aux=2)
    return [_desc(**zr), _desc(**zr)]


def _plans(reach):
    return {(s[3], s[4]) for s in reach}


@pytest.mark.parametrize("B", [1, 32])
def test_reachable_finds_the_small_map_plans_of_the_f16_gru(lib, B):
    launch = _launch(lib, _f16_zr(), B, 64, 128, image=(B, 512, 1024))
    assert cl.relation(launch) == (1, 8)
    assert launch.sig[0] == "f16" and launch.sig[3:5] == ("tile4", "roles18")
    reach = cl.reachable(lib, launch)
    assert reach == cl.reachable(lib, launch)                                      # deterministic, lists in grid order
    assert launch.sig in reach and (launch.B, launch.H, launch.W) in reach[launch.sig]
    assert {("tile4", "roles18"), ("tile3", "roles17"), ("tile3", "roles18")} <= _plans(reach), _plans(reach)
    for sig, geos in reach.items():
        assert sig[:3] + sig[5:] == launch.sig[:3] + launch.sig[5:]                # only the plan moves
        assert len(set(geos)) == len(geos)
        for ragged in (False, True):
            b, h, w, made = cl.witness(lib, launch, sig, geos, ragged=ragged)
            assert cl.same_signature(lib, cl.with_signature(launch, sig, b, h, w), b, h, w), (sig, b, h, w)
            assert made == (ragged and (b, h, w) not in geos)
            if made:
                assert b >= 2 and h % 2 and w % 2
    small = next(s for s in reach if s[3:5] == ("tile3", "roles17"))
    b, h, w, made = cl.witness(lib, launch, small, reach[small], ragged=False)
    assert not made and b * h * w <= 1 * 16 * 32, (b, h, w)
    mid = next(s for s in reach if s[3:5] == ("tile3", "roles18"))
    assert (1, 60, 120) in reach[mid]                                              # one 480 x 960 pair


def test_reachable_finds_the_8_row_halo_tile_of_encoder_layer_1(lib):
    """3x3 64 -> 64 on fp32 rows, four images per pair at half resolution: the weights-stationary kernel (tile 6) at
    512 x 1024, the 8-row halo kernel (tile 5) where the half-resolution width is no multiple of 32."""
    launch = _launch(lib, [_desc(64, 64, 3, 3)], 4, 256, 512, image=(1, 512, 1024))
    assert cl.relation(launch) == (4, 2) and launch.sig[3] == "tile6"
    reach = cl.reachable(lib, launch)
    assert reach == cl.reachable(lib, launch)
    t5 = [s for s in reach if s[3] == "tile5"]
    assert len(t5) == 1 and all(h % 8 or w % 32 for _, h, w in reach[t5[0]]), t5
    assert (16, 68, 108) in reach[t5[0]] and (12, 80, 180) in reach[t5[0]]         # 4 x 136 x 216, 3 x 160 x 360
    assert all(w % 32 == 0 and h % 8 == 0 for s in reach if s[3] == "tile6" for _, h, w in reach[s])
    b, h, w, made = cl.witness(lib, launch, t5[0], reach[t5[0]])
    assert cl.same_signature(lib, cl.with_signature(launch, t5[0], b, h, w), b, h, w)
    assert made and b >= 2 and h % 8 and w % 32
    # with the fused statistics the blocks rule of same_signature applies and the witness keeps them
    st = _launch(lib, [_desc(64, 64, 3, 3, stats_out=FAKE, in_scale=FAKE, in_shift=FAKE, in_relu=1)], 4, 256, 512, image=(1, 512, 1024))
    reach = cl.reachable(lib, st)
    t5 = [s for s in reach if s[3] == "tile5"]
    assert len(t5) == 1
    b, h, w, made = cl.witness(lib, st, t5[0], reach[t5[0]])
    assert cl.same_signature(lib, cl.with_signature(st, t5[0], b, h, w), b, h, w)


def test_reachable_drops_sizes_the_divisor_does_not_divide_and_refusals(lib):
    launch = _launch(lib, [_desc(256, 128, 3, 3, split=True)], 1, 17, 27, image=(1, 136, 216))
    assert cl.relation(launch) == (1, 8)
    reach = cl.reachable(lib, launch, grid=((1, 136, 216), (1, 100, 216), (1, 136, 220), (2, 512, 1024)))
    assert sorted(g for geos in reach.values() for g in geos) == [(1, 17, 27), (2, 64, 128)]
    # fused statistics on the generic kernel exist only where its pixel tiles do not straddle images: other sizes are left out
    st = _launch(lib, [_desc(64, 96, 3, 3, stride=2, stats_out=FAKE)], 4, 128, 256, image=(1, 512, 1024))
    assert st.sig[3] == "tile7"
    for sig, geos in cl.reachable(lib, st).items():
        for b, h, w in geos:
            assert cl.same_signature(lib, cl.with_signature(st, sig, b, h, w), b, h, w)
    assert all(g != (4, 34, 54) for geos in cl.reachable(lib, st).values() for g in geos)     # 34 * 54 % 128 != 0


def test_relation_needs_whole_images_and_a_whole_divisor(lib):
    d = [_desc(256, 128, 3, 3, split=True)]
    assert cl.relation(_launch(lib, d, 6, 64, 128, image=(3, 512, 1024))) == (2, 8)
    for geo, image in (((3, 64, 128), (2, 512, 1024)), ((1, 64, 128), (1, 500, 1024)), ((1, 64, 128), (1, 512, 512)),
                       ((1, 64, 128), (2, 512, 1024)), ((1, 64, 128), None)):
        launch = _launch(lib, d, *geo, image=image)
        with pytest.raises(ValueError) as e:
            cl.relation(launch)
        assert cl.sig_str(launch.sig) in str(e.value)


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


# ---------------------------------------------------------------------------------------------------------------------
# ragged tiles of the 8-row halo kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tile5_case(lib):
    """Encoder layer 1 as fnet launches it (3x3 64 -> 64 on fp32 rows, folded input norm + ReLU, fused statistics) on the
    8-row halo tile at H = 13 (a 5-row last tile) and W = 41 (a 9-column last strip), with its exact result."""
    B, H, W = 128, 13, 41
    d = _desc(64, 64, 3, 3, in_scale=FAKE, in_shift=FAKE, in_relu=1, stats_out=FAKE)
    launch = _launch(lib, [d], B, H, W)
    assert launch.sig[3] == "tile5"
    case = cl.build_case(lib, launch, B, H, W, torch.device("cpu"), seed=13)
    return case, cl.reference(case)


def _store(case, acc_of):
    """Fills the case's buffers as a kernel would whose accumulators are acc_of(exact accumulators [B, H, W, cout]) -- NaN
    marks a pixel it never writes (the sentinel stays) --, statistics partials consistent with what it wrote."""
    g = case.groups[0]
    T = g["T"]

    def conv(x, w, B, H, W, stride):
        r = dict(cl.conv_fp64(x, w, B, H, W, stride))
        r["acc"] = acc_of(r["acc"].view(B, H, W, -1).clone()).reshape(B * H * W, -1)
        return r
    val = cl.reference(case, conv=conv)[0]["out"]["ref"]
    out = torch.full_like(T["out"], cl.SENT_F32)
    live = out[:, g["off_out"]:g["off_out"] + g["cout"]]
    live.copy_(torch.where(torch.isnan(val), torch.full_like(val, cl.SENT_F32), val).float())
    T["out"].copy_(out)
    y = live.double().view(case.B, -1, g["cout"])
    T["stats"].zero_()
    T["stats"][:, 0, :, 0], T["stats"][:, 0, :, 1] = y.sum(1), (y * y).sum(1)


def _nan_from(rows=None, cols=None):
    def f(acc):
        acc[:, rows if rows is not None else slice(None), cols if cols is not None else slice(None)] = float("nan")
        return acc
    return f


def _stale_rows(acc):                           # the last tile's rows still hold the tile above
    acc[:, 8:13] = acc[:, 0:5]
    return acc


def _stale_cols(acc):                           # the last strip's columns still hold the strip before
    acc[:, :, 32:41] = acc[:, :, 0:9]
    return acc


def _zero_cols(acc):                            # the last strip's accumulators never saw a product: bias only
    acc[:, :, 32:41] = 0
    return acc


def test_tile5_exact_result_passes(tile5_case):
    case, refs = tile5_case
    _store(case, lambda acc: acc)
    fails, worst = cl.check_case(case, refs)
    assert not fails, fails
    assert worst["elem"] <= 0.05 and worst["agg"] <= 0.05, worst         # fp32 rounding of the stored value only


@pytest.mark.parametrize("fault", [_nan_from(rows=slice(8, 13)), _stale_rows, _nan_from(cols=slice(32, 41)), _stale_cols, _zero_cols],
                         ids=["last-row-tile-unwritten", "last-row-tile-stale", "last-strip-unwritten", "last-strip-stale", "last-strip-no-products"])
def test_tile5_partial_tiles_have_teeth(tile5_case, fault):
    """A kernel that loses the rows of the last partial 8-row tile or the columns of the last partial 32-column strip fails
    check_case on the output itself (the statistics are kept consistent with what it stored)."""
    case, refs = tile5_case
    _store(case, fault)
    fails, worst = cl.check_case(case, refs)
    assert any("group 0 out" in f and "per-element" in f for f in fails), fails
    assert any("group 0 out" in f and "aggregate" in f for f in fails), fails
    assert worst["elem"] > 10 and worst["agg"] > 10, worst
    _store(case, lambda acc: acc)                                         # leave the shared case exact
    assert not cl.check_case(case, refs)[0]
