"""GPU: the fp16 update blocks of ``args.mixed_precision`` (PF_PREC_F16).  Kernel parity of every geometry the engine launches
in that mode against F.conv2d of fp16-rounded operands with fp64 accumulation; the f16-map producers against torch's .half() of
their own fp32 outputs; the whole forward against the CPU oracle with exactly engine.F16_CONVS rounded to fp16; and the API
behaviour (graph = eager, lists, init_flow, switching the flag, the training forward).  Run with ``-m gpu`` on an MI355X."""
import argparse

import pytest
import torch
import torch.nn.functional as F

import golden_cases as gc
import priorflow_oracle as po

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def params():
    from prior_flow_amd.modules import state_dict_shapes
    return gc.det_state_dict(state_dict_shapes())


@pytest.fixture(scope="module")
def lib():
    from prior_flow_amd import _lib
    return _lib.load()


def make_model(params, mixed):
    from prior_flow_amd.prior_raft import PriOr_RAFT
    m = PriOr_RAFT(argparse.Namespace(mixed_precision=mixed, dropout=0.0))
    m.load_state_dict(params, strict=True)
    return m.cuda().eval()


def nchw(rows, B, H, W):
    return rows.reshape(B, H, W, -1).permute(0, 3, 1, 2)


def f16_ref_conv(x_rows, w, b, B, H, W, kh, kw):
    """fp64 conv of fp16-rounded channel-last rows x [B*H*W][cin] and weight w [cout][cin][kh][kw] (+ fp32 bias)."""
    x = nchw(x_rows.half().double(), B, H, W)
    y = F.conv2d(x, w.half().double(), b.double(), padding=(kh // 2, kw // 2))
    return y.permute(0, 2, 3, 1).reshape(B * H * W, -1)


def close(got, ref, tol=1e-5):
    err = (got.double().cpu() - ref.cpu()).abs().max().item()
    scale = max(ref.abs().max().item(), 1.0)
    assert err <= tol * scale, (err, scale)


def rand_rows(g, rows, c, scale=1.0):
    return (torch.randn(rows, c, generator=g) * scale).float()


# ---- kernel parity --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H8,W8", [(1, 64, 128), (2, 37, 53)])
def test_f16_convs_match_fp64_of_rounded_operands(lib, B, H8, W8):
    """3x3 128 -> 64 / 256 -> 128|192 (two groups) / 272 -> 124 (320-wide map) / 128 -> 256 heads, 1x5 and 5x1 GRU_ZR / GRU_Q
    with `pre` and the aux / out maps, co_groups; on a full map and an odd map with partial tiles."""
    from prior_flow_amd import _lib
    from prior_flow_amd.engine import Conv, f16_map, pack_mfma
    g = torch.Generator().manual_seed(7)
    rows = B * H8 * W8

    def conv_of(cout, cin, kh, kw, cin_to=0):
        w = torch.randn(cout, cin, kh, kw, generator=g) / (cin * kh * kw) ** 0.5
        b = torch.randn(cout, generator=g) * 0.1
        wp, bp = pack_mfma(w.to(DEV), b.to(DEV), cin_to)
        return Conv(wp, bp, kh, kw, max(cin, cin_to), cout, _lib.PREC_F16), w, b

    def map_of(x, width):
        m = f16_map(rows, width, DEV)
        lib.split_f16(x.to(DEV), m)
        return m

    roles_seen = set()

    def run(descs):
        roles_seen.add(lib.conv2d_roles(descs, B, H8, W8))
        lib.conv2d(descs, B, H8, W8, like)
    like = torch.zeros(1, device=DEV)

    # 3x3 relu, single group, f16 map + fp32 out at an offset
    for cin, cout in ((128, 64), (128, 256)):
        cv, w, b = conv_of(cout, cin, 3, 3)
        x = rand_rows(g, rows, cin)
        out = torch.zeros(rows, 320, device=DEV)
        outs = f16_map(rows, 320, DEV)
        run([cv.desc(None, 0, cin, out, 64, _lib.EPI_RELU, in0s=map_of(x, cin), outs=outs)])
        ref = f16_ref_conv(x, w, b, B, H8, W8, 3, 3).clamp_min(0)
        close(out[:, 64:64 + cout], ref)
        assert torch.equal(outs[:, 64:64 + cout], out[:, 64:64 + cout].half())
        assert not outs[:, :64].any() and not outs[:, 64 + cout:].any()
    # the heads: flow_head.conv1 and mask.0 (3x3 128 -> 256) on one input as two groups (the 256 px x 64 channel tile at B = 1)
    heads = [conv_of(256, 128, 3, 3), conv_of(256, 128, 3, 3)]
    x = rand_rows(g, rows, 128)
    xm = map_of(x, 128)
    outs = [torch.zeros(rows, 256, device=DEV) for _ in heads]
    run([c.desc(None, 0, 128, o, 0, _lib.EPI_RELU, in0s=xm) for (c, _, _), o in zip(heads, outs)])
    for (c, w, b), o in zip(heads, outs):
        close(o, f16_ref_conv(x, w, b, B, H8, W8, 3, 3).clamp_min(0))
    # two groups 256 -> 128 | 192, and the same launch as one group with co_groups = 1
    cvs = [conv_of(128, 256, 3, 3), conv_of(192, 256, 3, 3)]
    xs = [rand_rows(g, rows, 256, 2.0) for _ in cvs]
    ms = [map_of(x, 256) for x in xs]
    outs = [torch.zeros(rows, 192, device=DEV) for _ in cvs]
    run([c.desc(None, 0, 256, o, 0, _lib.EPI_RELU, in0s=m) for (c, _, _), o, m in zip(cvs, outs, ms)])
    for (c, w, b), o, x in zip(cvs, outs, xs):
        close(o[:, :c.cout], f16_ref_conv(x, w, b, B, H8, W8, 3, 3).clamp_min(0))
    o2 = torch.zeros(rows, 192, device=DEV)
    d = cvs[0][0].desc(None, 0, 256, o2, 0, _lib.EPI_RELU, in0s=ms[0])
    d.co_groups = 1
    run([d])
    assert torch.equal(o2, outs[0])
    # conv_A: 272 channels in a 320-wide map (zero tail), output map at channel 128 of the GRU input
    cv, w, b = conv_of(124, 272, 3, 3)
    x = rand_rows(g, rows, 272)
    xm = map_of(x, 272)
    xo = f16_map(rows, 256, DEV)
    out = torch.zeros(rows, 124, device=DEV)
    run([cv.desc(None, 0, 272, out, 0, _lib.EPI_RELU, in0s=xm, outs=None)])
    close(out, f16_ref_conv(x, w, b, B, H8, W8, 3, 3).clamp_min(0))
    run([cv.desc(None, 0, 272, None, 128, _lib.EPI_RELU, in0s=xm, outs=xo)])
    assert torch.equal(xo[:, 128:252], out.half()) and not xo[:, :128].any()
    # GRU half-steps with the hoisted context: [h | motion] = net map (128) + channels 128..255 of the GRU-input map
    for kh, kw in ((1, 5), (5, 1)):
        zr, wzr, bzr = conv_of(256, 256, kh, kw)
        q, wq, bq = conv_of(128, 256, kh, kw)
        h = rand_rows(g, rows, 128, 0.5).to(DEV)
        xin = rand_rows(g, rows, 256)
        pre = rand_rows(g, rows, 384, 0.3).to(DEV)
        hm, xm = map_of(h.cpu(), 128), map_of(xin, 256)
        z = torch.zeros(rows, 128, device=DEV)
        rhm = f16_map(rows, 128, DEV)
        run([zr.desc(None, 0, 128, z, 0, _lib.EPI_GRU_ZR, off1=128, c1=128, h=h, in0s=hm, in1s=xm, auxs=rhm, pre=pre, off_pre=0)])
        hx = torch.cat([h.cpu(), xin[:, 128:]], 1)
        a = f16_ref_conv(hx, wzr, bzr, B, H8, W8, kh, kw) + pre[:, :256].cpu().double()
        close(z, torch.sigmoid(a[:, :128]))
        rh_ref = torch.sigmoid(a[:, 128:]) * h.cpu().double()
        close(rhm.float(), rh_ref, 1e-3)                 # fp16 storage of r*h: one rounding
        hn = torch.zeros(rows, 128, device=DEV)
        hnm = f16_map(rows, 128, DEV)
        run([q.desc(None, 0, 128, hn, 0, _lib.EPI_GRU_Q, off1=128, c1=128, h=h, z=z, in0s=rhm, in1s=xm, outs=hnm,
                    pre=pre, off_pre=256)])
        qa = f16_ref_conv(torch.cat([rhm.float().cpu(), xin[:, 128:]], 1), wq, bq, B, H8, W8, kh, kw) + pre[:, 256:].cpu().double()
        zz = z.cpu().double()
        close(hn, (1 - zz) * h.cpu().double() + zz * torch.tanh(qa))
        assert torch.equal(hnm, hn.half())
    if (B, H8, W8) == (1, 64, 128):
        assert roles_seen == {17, 18}, roles_seen


# ---- producers of the f16 maps --------------------------------------------------------------------------------------------
def test_f16_producers_write_half_of_their_fp32_output(lib, params):
    """pf_split_f16, pf_motion_prep_f16, pf_conf_stem_f16, pf_conv2d_direct_group_f16 and pf_dccl_combine_conv1x1_f16 write
    torch's .half() of what their fp32 forms write, bit for bit, and nothing past the logical width."""
    from prior_flow_amd import _lib
    from prior_flow_amd.engine import CORR_CH, Workspace, f16_map, pack_update_blocks
    m = make_model(params, True)
    P = pack_update_blocks(m.ODDC, m.update_block, _lib.PREC_F16)
    B, H, W = 1, 128, 256
    ws = Workspace(lib, B, H, W, torch.device(DEV), f16=True)
    rows = B * ws.N
    g = torch.Generator().manual_seed(3)
    # split_f16 of a column slice, including values past fp16's normal range
    x = rand_rows(g, rows, 256, 3.0)
    x[:7, 0] = torch.tensor([1e-6, -3e-8, 7e4, -1e5, 65519.0, 65520.0, 2.0 ** -25])
    x = x.to(DEV)
    mp = f16_map(rows, 192, DEV)
    lib.split_f16(x[:, :136], mp)
    assert torch.equal(mp[:, :136], x[:, :136].half()) and not mp[:, 136:].any()
    # motion prep: flows into the GRU-input maps
    ws.c1a.copy_(ws.coords0 + torch.randn(ws.c1a.shape, generator=g).to(DEV))
    ws.c1b.copy_(ws.coords0 + torch.randn(ws.c1b.shape, generator=g).to(DEV))
    ws.f["f1a"].copy_(rand_rows(g, rows, 256).to(DEV))
    ws.f["f2a"].copy_(rand_rows(g, rows, 256).to(DEV))
    xa, xb = torch.zeros(rows, 256, device=DEV), torch.zeros(rows, 256, device=DEV)
    lib.motion_prep(ws.c1a, ws.c1b, ws.g_a2b_8, ws.g_b2a_8, ws.f["f1a"], ws.f["f2a"], ws.flow4_a, ws.flow2_b, ws.conf_in,
                    xa, 252, xb, 254)
    lib.motion_prep(ws.c1a, ws.c1b, ws.g_a2b_8, ws.g_b2a_8, ws.f["f1a"], ws.f["f2a"], ws.flow4_a, ws.flow2_b, ws.conf_in,
                    None, 252, None, 254, xa_split=ws.x_a_s, xb_split=ws.x_b_s)
    assert torch.equal(ws.x_a_s[:, 252:], xa[:, 252:].half()) and torch.equal(ws.x_b_s[:, 254:], xb[:, 254:].half())
    assert not ws.x_a_s[:, :252].any() and not ws.x_b_s[:, :254].any()
    # confidence stem -> cat_a[256:272] (320-wide map)
    c1, c2 = P["a.cf1"], P["a.cf2"]
    cat = torch.zeros(rows, 272, device=DEV)
    lib.conf_stem(ws.conf_in, 0, c1.w, c1.b, c2.w, c2.b, cat, 256, B, ws.H8, ws.W8)
    lib.conf_stem(ws.conf_in, 0, c1.w, c1.b, c2.w, c2.b, None, 256, B, ws.H8, ws.W8, out_split=ws.cat_a_s)
    assert torch.equal(ws.cat_a_s[:, 256:272], cat[:, 256:].half()) and not ws.cat_a_s[:, 272:].any()
    # 7x7 flow stems (MFMA form) -> t maps
    st = [(P["a.f1a"], ws.flow4_a, 0), (P["a.f1b"], ws.flow4_a, 2), (P["b.f1"], ws.flow2_b, 0)]
    outs = [torch.zeros(rows, 128, device=DEV) for _ in st]
    dc = st[0][0]
    lib.conv2d_direct_group([(x_, o_, c.w, c.b, out, 0) for (c, x_, o_), out in zip(st, outs)], dc.cin, dc.cout, dc.kh, dc.kw,
                            True, B, ws.H8, ws.W8)
    tms = [ws.t_a_s, ws.t_ba_s, ws.t_b_s]
    lib.conv2d_direct_group([(x_, o_, c.w, c.b, None, 0, t) for (c, x_, o_), t in zip(st, tms)], dc.cin, dc.cout, dc.kh, dc.kw,
                            True, B, ws.H8, ws.W8)
    for t, o in zip(tms, outs):
        assert torch.equal(t, o.half())
    # fused lookup combine + convc1 (bf16x3 arithmetic) -> c1 maps
    own, raw = rand_rows(g, rows, CORR_CH).to(DEV), rand_rows(g, rows, CORR_CH).to(DEV)
    out = torch.zeros(rows, 256, device=DEV)
    lib.dccl_combine_conv1x1([(own, raw, ws.g_b2a_8, P["a.c1"], out, 0)], B, ws.H8, ws.W8)
    lib.dccl_combine_conv1x1([(own, raw, ws.g_b2a_8, P["a.c1"], None, 0, ws.c1_a_s)], B, ws.H8, ws.W8)
    assert torch.equal(ws.c1_a_s, out.half())
    torch.cuda.synchronize()


# ---- the forward against the emulation ------------------------------------------------------------------------------------
def emulated_oracle(monkeypatch):
    """The CPU oracle with the convolutions of engine.F16_CONVS on fp16-rounded inputs and weights (fp32 accumulation)."""
    from prior_flow_amd.engine import F16_CONVS
    plain = po._conv

    def conv(p, name, x, pad):
        if name in F16_CONVS:
            return F.conv2d(x.half().float(), p[name + ".weight"].half().float(), p[name + ".bias"], padding=pad)
        return plain(p, name, x, pad)
    return plain, conv


@pytest.mark.parametrize("B,H,W", [(1, 128, 256), (2, 256, 512)])
def test_forward_matches_the_fp16_emulation(params, monkeypatch, B, H, W):
    """e_emu = EPE(GPU, emulation) must sit at the order-noise level, well under e_ref = EPE(emulation, fp32 oracle): today's
    bf16x3 path gives e_emu ~ e_ref."""
    m = make_model(params, True)
    i1, i2 = gc.synthetic_pair(B, H, W)
    with torch.no_grad():
        got = m(i1.cuda(), i2.cuda(), iters=12, test_mode=True).cpu()
    plain, conv = emulated_oracle(monkeypatch)
    ref = po.forward(params, i1, i2, iters=12, test_mode=True)
    monkeypatch.setattr(po, "_conv", conv)
    emu = po.forward(params, i1, i2, iters=12, test_mode=True)
    monkeypatch.setattr(po, "_conv", plain)
    pick = lambda r: r[0] if isinstance(r, (tuple, list)) else r          # noqa: E731
    ref, emu = pick(ref), pick(emu)
    e_emu = float(po.epe(got, emu).mean())
    e_ref = float(po.epe(emu, ref).mean())
    print(f"{B}x{H}x{W}: EPE(GPU f16, emulation) {e_emu:.3e}  EPE(emulation, fp32 oracle) {e_ref:.3e}")
    assert e_emu <= 0.4 * e_ref and e_emu <= 1.5e-3, (e_emu, e_ref)


# ---- API behaviour ----------------------------------------------------------------------------------------------------------
def test_graph_replay_equals_eager_in_f16_mode(params):
    m = make_model(params, True)
    i1, i2 = gc.synthetic_pair(1, 128, 256)
    with torch.no_grad():
        m.use_graph = True
        a = m(i1.cuda(), i2.cuda(), iters=12, test_mode=True)
        b = m(i1.cuda(), i2.cuda(), iters=12, test_mode=True)
        m.use_graph = False
        c = m(i1.cuda(), i2.cuda(), iters=12, test_mode=True)
    assert torch.equal(a, b) and torch.equal(a, c)


def test_lists_and_init_flow_in_f16_mode(params):
    m = make_model(params, True)
    i1, i2 = gc.synthetic_pair(1, 128, 256)
    with torch.no_grad():
        pa, pb = m(i1.cuda(), i2.cuda(), iters=4)
        assert len(pa) == 4 and len(pb) == 4 and tuple(pa[-1].shape) == (1, 2, 128, 256)
        assert all(torch.isfinite(p).all() for p in pa + pb)
        init = torch.full((1, 2, 16, 32), 0.5, device=DEV)
        f0 = m(i1.cuda(), i2.cuda(), iters=4, test_mode=True)
        f1 = m(i1.cuda(), i2.cuda(), iters=4, init_flow=init, test_mode=True)
        assert torch.isfinite(f1).all() and not torch.equal(f0, f1)
        # test_mode=False's last prediction is test_mode=True's flow (same arithmetic, eager)
        m.use_graph = False
        assert torch.equal(pa[-1], m(i1.cuda(), i2.cuda(), iters=4, test_mode=True))


def test_switching_the_flag_back_is_bitwise_the_default(params):
    i1, i2 = gc.synthetic_pair(1, 128, 256)
    m = make_model(params, True)
    fresh = make_model(params, False)
    with torch.no_grad():
        f16 = m(i1.cuda(), i2.cuda(), iters=12, test_mode=True)
        m.args.mixed_precision = False
        back = m(i1.cuda(), i2.cuda(), iters=12, test_mode=True)
        want = fresh(i1.cuda(), i2.cuda(), iters=12, test_mode=True)
        assert torch.equal(back, want) and not torch.equal(f16, want)
        m.args.mixed_precision = True                           # and again: the f16 result comes back
        assert torch.equal(m(i1.cuda(), i2.cuda(), iters=12, test_mode=True), f16)
    from prior_flow_amd import _lib
    fresh.precision = _lib.PREC_F16                             # the attribute selects the same mode
    with torch.no_grad():
        assert torch.equal(fresh(i1.cuda(), i2.cuda(), iters=12, test_mode=True), f16)


def test_training_forward_ignores_the_flag(params):
    i1, i2 = gc.synthetic_pair(1, 128, 256)
    outs = []
    for mixed in (False, True):
        m = make_model(params, mixed).train()
        m.freeze_bn()
        pa, pb = m(i1.cuda(), i2.cuda(), iters=3)
        (pa[-1].square().mean() + pb[-1].square().mean()).backward()
        outs.append([p.detach() for p in pa + pb])
    assert all(torch.equal(a, b) for a, b in zip(*outs))
