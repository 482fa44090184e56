"""Flow rendering on an MI355X: pf_order_stat against np.sort, pf_flow_render and pf_cycle_warp against the
reference's stored results (tests/golden/flow_viz.npz), the float64 restatement (tests/flow_viz_ref.py) and the host emulation,
FlowRenderer inside a captured graph, and the composition with FlowStream and demo_image.  Run with ``-m gpu``.

Measured on an MI355X: colour bytes against the reference's differ on 0 / 1.0e-5 / 0 (omni) and 0 / 2.0e-5 / 0
(plane) of the values at 64x128 / 128x256 / 136x216, never by more than 1, and were observed equal to the host emulation's on every
byte (the test holds them to the colour bar: the two sides use different sin / atan2 implementations); against
float64 at 512x1024, B = 2: 1.1e-4 (omni), 5.1e-6 (plane); length map 2.4e-7 - 3.6e-7 from calculate_veclen_spherical; warp 0 from
my_cycle_warp at the three fixture sizes and bit for bit equal to the emulation, 3.1e-5 - 3.4e-5 from float64; mean_err 1e-8 - 5e-8 relative."""
import argparse
import os

import numpy as np
import pytest
import torch

import flow_viz_cases as fc
import flow_viz_checks as ck
import flow_viz_ref as fr
import golden_cases as gc

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def lib():
    from prior_flow_amd._lib import load
    return load()


@pytest.fixture(scope="module")
def gold():
    return ck.golden()


@pytest.fixture(scope="module")
def emu():
    import emu_lib
    return emu_lib.load()


# ---- the order statistic ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2, 8])
@pytest.mark.parametrize("kind", ck.OS_KINDS)
def test_order_stat_is_np_sort_bit_for_bit(lib, kind, B):
    n = 512 * 1024
    x = ck.os_input(kind, B, n, seed=B + 40)
    for k in ck.os_ranks(n):
        outs = ck.run_order_stat(lib, x, k, device=DEV, repeats=5)
        want = ck.os_expected(x, k)
        for got in outs:                                                   # five launches, identical
            assert got.view(np.uint32).tolist() == want.view(np.uint32).tolist(), (kind, B, k, got, want)


@pytest.mark.parametrize("n", [1, 7, 255, 29376, 1000003])
def test_order_stat_odd_sizes(lib, n):
    x = ck.os_input("random", 3, n, seed=n % 89)
    for k in sorted({0, n // 2, n - 1}):
        got = ck.run_order_stat(lib, x, k, device=DEV)
        assert got.view(np.uint32).tolist() == ck.os_expected(x, k).view(np.uint32).tolist()


@pytest.mark.parametrize("kind", ck.OS_CAPPED_KINDS)
def test_order_stat_beyond_the_grid_cap(lib, kind):
    """n = 4 200 000 > 2048 workgroups x 256 threads x 8 items: pf_os_blocks caps the grid of the three selection passes and
    some threads go round their loop a ninth time (no smaller case reaches the cap: tests/test_launch_paths.py).  B = 2, the
    ranks of ck.os_ranks, bit for bit against np.sort."""
    import launch_paths as lp
    n, B = ck.OS_CAPPED_N, 2
    want, launched, trips = lp.os_grid(n, lp.OS_SELECT_PER)
    print(f"[flow_viz] order statistic n = {n}: {launched} of {want} workgroups wanted per image, {trips} trips")
    assert launched < want and trips == lp.OS_SELECT_PER + 1
    x = ck.os_input(kind, B, n, seed=61)
    first_trips = lp.OS_MAX_BLOCKS * lp.ELEM_BLOCK * lp.OS_SELECT_PER
    if kind == "tied":                                  # the two largest ranks are values that only the ninth trip reads
        x[:, first_trips:] = np.float32(1.0)
    s = np.sort(x, axis=1)
    assert not np.isnan(s).any() and (kind != "tied" or (len(np.unique(s)) <= 17 and s[0, -1] == 1.0 and (x[:, :first_trips] < 1).all()))
    # without the ninth trip's values the rank 0.95 n falls on another value
    assert (np.sort(x[:, :first_trips], axis=1)[:, int(0.95 * n)] != s[:, int(0.95 * n)]).all() or kind == "tied"
    for k in ck.os_ranks(n):
        got = ck.run_order_stat(lib, x, k, device=DEV)
        assert got.view(np.uint32).tolist() == s[:, k].view(np.uint32).tolist(), (kind, k, got, s[:, k])


def test_order_stat_nan_rules(lib):
    x = np.array([[3.0, np.nan, 1.0, np.nan, 2.0], [np.nan] * 5, [0.5, np.inf, np.nan, 0.25, 0.0]], np.float32)
    assert ck.run_order_stat(lib, x, 2, device=DEV).tolist() == [3.0, 0.0, 0.5]
    assert ck.run_order_stat(lib, x, 4, device=DEV).tolist() == [3.0, 0.0, np.inf]
    assert ck.run_order_stat(lib, x, 0, device=DEV).tolist() == [1.0, 0.0, 0.0]


# ---- render ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["hwc", "chw"])
@pytest.mark.parametrize("H,W", fc.SIZES)
def test_render_matches_the_reference(lib, emu, gold, H, W, layout):
    flow = ck.fixture_flow(gold, H, W)
    hwc = (lambda a: a) if layout == "hwc" else (lambda a: a.transpose(0, 2, 3, 1))
    img, length, clip = ck.run_render(lib, flow, "omni", layout=layout, device=DEV)
    d = np.abs(length.astype(np.float64) - gold[f"sd_{H}x{W}"]).max()
    print(f"[flow_viz] device len against calculate_veclen_spherical {H}x{W}: {d:.3e}")
    assert d <= ck.SD_ATOL
    want_clip = np.array([np.sort(length[b], axis=None)[int(0.95 * H * W)] for b in range(len(flow))], np.float32)
    assert clip.view(np.uint32).tolist() == want_clip.view(np.uint32).tolist()
    ck.colour_figures(hwc(img), gold[f"omni_{H}x{W}"], f"device omni {layout} {H}x{W}")
    e_img = ck.run_render(emu, flow, "omni", layout=layout)[0]
    ck.colour_figures(img, e_img, f"device omni {layout} {H}x{W} against the emulation")
    imgp, lenp, clipp = ck.run_render(lib, flow, "plane", layout=layout, device=DEV)
    assert clipp.view(np.uint32).tolist() == lenp.reshape(len(flow), -1).max(1).view(np.uint32).tolist()
    ck.colour_figures(hwc(imgp), gold[f"plane_{H}x{W}"], f"device plane {layout} {H}x{W}")


@pytest.mark.parametrize("mode", ["omni", "plane"])
def test_render_one_pixel_path_matches_float64(lib, mode):
    """W % 4 != 0: one pixel per thread."""
    flow = fc.make_flow(2, 64, 130, seed=21)
    for layout in ("hwc", "chw"):
        img = ck.run_render(lib, flow, mode, layout=layout, device=DEV)[0]
        img = img if layout == "hwc" else img.transpose(0, 2, 3, 1)
        ck.colour_figures(img, fr.render(flow, mode), f"device {mode} {layout} 64x130 against float64")


@pytest.mark.parametrize("mode", ["omni", "plane"])
def test_render_512x1024_matches_float64(lib, mode):
    flow, _ = ck.big_case()
    for layout, bgr in (("hwc", False), ("chw", True)):
        img, length, clip = ck.run_render(lib, flow, mode, layout=layout, bgr=bgr, device=DEV)
        img = img if layout == "hwc" else img.transpose(0, 2, 3, 1)
        ck.colour_figures(img, fr.render(flow, mode, bgr=bgr), f"device {mode} {layout} bgr={bgr} 512x1024 B=2 against float64")
    if mode == "omni":
        assert np.abs(length - fr.veclen_spherical(flow)).max() <= ck.SD_ATOL


@pytest.mark.parametrize("mode,layout", [("omni", "hwc"), ("plane", "chw")])
@pytest.mark.parametrize("H,W", ck.RENDER_CAPPED)
def test_render_beyond_the_grid_cap_matches_float64(lib, mode, layout, H, W):
    """258 x 2034 (W % 4 != 0: one pixel per thread, 524 772 pixels) and 1026 x 2048 (four pixels per thread, 525 312 quads): the
    grids of the length pass and of the colour kernel are capped at 2048 workgroups and their first threads make a second trip,
    which holds the last 484 pixels and the last two rows.  Under the colour bar against float64; the length map to SD_ATOL."""
    import launch_paths as lp
    (form, (want, launched, trips)), = lp.render_grids(H, W).items()
    print(f"[flow_viz] render {H}x{W}, {form}: {launched} of {want} workgroups wanted, {trips} trips")
    assert launched < want and trips == 2
    flow = fc.make_flow(1, H, W, seed=27)
    img, length, clip = ck.run_render(lib, flow, mode, layout=layout, device=DEV)
    img = img if layout == "hwc" else img.transpose(0, 2, 3, 1)
    ck.colour_figures(img, fr.render(flow, mode), f"device {mode} {layout} {H}x{W} against float64")
    want_len = fr.lengths(flow, mode)
    d = np.abs(length - want_len).max()
    print(f"[flow_viz] device len {mode} {H}x{W} against float64: {d:.3e}")
    # omni: the bar of the great-circle length; plane: sqrtf(u u + v v), four roundings of half an ulp at most
    assert d <= (ck.SD_ATOL if mode == "omni" else 2.0 ** -22 * want_len.max())
    k = int(0.95 * H * W) if mode == "omni" else H * W - 1          # the clip is the device's own length map's order statistic
    assert clip.view(np.uint32).tolist() == np.sort(length[0], axis=None)[k:k + 1].view(np.uint32).tolist()
    tail = slice(lp.OS_MAX_BLOCKS * lp.ELEM_BLOCK * (4 if form == "four_pixel" else 1), None)      # the second trip's pixels
    assert len(np.unique(img.reshape(-1, 3)[tail], axis=0)) > 10


@pytest.mark.parametrize("mode", ["omni", "plane"])
@pytest.mark.parametrize("layout", ["hwc", "chw"])
def test_vector_and_scalar_paths_are_equal(lib, mode, layout):
    """The same 136x216 flows 16-byte aligned (four pixels per thread) and 4 bytes off (one pixel per thread): the same bits."""
    flow = fc.make_flow(2, 136, 216, seed=23)
    for bgr in (False, True):
        a = ck.run_render(lib, flow, mode, layout=layout, bgr=bgr, device=DEV, offset=4)
        b = ck.run_render(lib, flow, mode, layout=layout, bgr=bgr, device=DEV, offset=1)
        for p, q in zip(a, b):
            assert np.array_equal(p.view(np.uint8), q.view(np.uint8))


def test_hand_cases(lib):
    for mode in ("omni", "plane"):
        assert (ck.run_render(lib, np.zeros((2, 2, 16, 32), np.float32), mode, device=DEV)[0] == 255).all()
    flow = fc.make_flow(2, 64, 128, seed=25)
    bad = flow.copy()
    spots = [(0, 0, 5, 7, np.nan), (0, 1, 20, 100, np.inf), (1, 0, 63, 127, -np.inf), (1, 1, 30, 0, np.nan)]
    for b, c, y, x, v in spots:
        bad[b, c, y, x] = v
    for mode in ("omni", "plane"):
        img = ck.run_render(lib, bad, mode, device=DEV)[0]
        assert (img.reshape(-1, 3).max(1) == 0).sum() == len(spots)
        for b, c, y, x, v in spots:
            assert img[b, y, x].tolist() == [0, 0, 0]
        ck.colour_figures(img, fr.render(bad, mode), f"device non-finite, {mode}")
    x = fc.make_image(2, 3, 16, 32, seed=3)
    pan = np.zeros((2, 2, 16, 32), np.float32)
    pan[:, 0] = 5
    assert np.array_equal(ck.run_warp(lib, x, pan, device=DEV)[0], np.roll(x, -5, axis=3))


# ---- warp ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_ref", [False, True])
@pytest.mark.parametrize("H,W,C", ck.WARP_CASES)
def test_warp_matches_the_reference(lib, emu, gold, H, W, C, with_ref):
    flow = ck.fixture_flow(gold, H, W)[:1]
    img = gold[f"image_{H}x{W}"].astype(np.float32)[:, :C].copy()
    ref = fc.make_image(1, C, H, W, seed=31) if with_ref else None
    got, err = ck.run_warp(lib, img, flow, ref=ref, device=DEV)
    d = np.abs(got.astype(np.float64) - gold[f"warp_{H}x{W}"][:, :C]).max()
    e_got, e_err = ck.run_warp(emu, img, flow, ref=ref)
    bitwise = np.array_equal(got, e_got) and (err is None or np.array_equal(err, e_err))
    print(f"[flow_viz] device warp {H}x{W} C={C} ref={with_ref} against my_cycle_warp: {d:.3e}; equal to the emulation bit for bit: {bitwise}")
    assert d <= ck.WARP_ATOL
    assert bitwise                       # the same PF_HD code, no contraction on either side


@pytest.mark.parametrize("H,W,B", [(128, 256, 1), (136, 216, 1), (64, 130, 2), (512, 1024, 2)])
def test_warp_matches_float64(lib, emu, H, W, B):
    flow = fc.make_flow(B, H, W, seed=33)
    for C in (1, 3):
        img = fc.make_image(B, C, H, W, seed=33)
        ref = fc.make_image(B, C, H, W, seed=34)
        got, err = ck.run_warp(lib, img, flow, ref=ref, device=DEV)
        d = np.abs(got - fr.cycle_warp(img, flow)).max()
        print(f"[flow_viz] device warp {H}x{W} B={B} C={C} against float64: {d:.3e}")
        assert d <= ck.WARP_ATOL
        want_err, want_mean = fr.photometric(ref, got)
        assert np.abs(err - want_err).max() <= 255 * 2.0 ** -22
        occ = (np.random.default_rng(35).random((B, H, W)) < 0.25).astype(np.uint8)
        for mask in (None, occ):
            got_mean = ck.run_masked_mean(lib, err, mask, device=DEV)
            want = fr.photometric(ref, got, mask)[1]
            rel = np.abs(got_mean - want).max() / want.max()
            print(f"[flow_viz] mean_err {H}x{W} B={B} C={C} mask={mask is not None}: relative difference {rel:.3e}")
            assert np.allclose(got_mean, want, rtol=ck.MEAN_ERR_RTOL, atol=0)
        if H * W <= 136 * 216:
            e_got, e_err = ck.run_warp(emu, img, flow, ref=ref)
            assert np.array_equal(got, e_got) and np.array_equal(err, e_err)
    full = np.ones((B, H, W), np.uint8)
    assert ck.run_masked_mean(lib, err, full, device=DEV).tolist() == [0.0] * B


# ---- FlowRenderer ----------------------------------------------------------------------------------------------------------
def test_python_interface(lib, gold):
    from prior_flow_amd import flow_viz
    from prior_flow_amd._lib import PfError
    flow = torch.from_numpy(ck.fixture_flow(gold, 64, 128)).cuda()
    one = flow_viz.omniflow_to_image(flow[0])
    assert tuple(one.shape) == (64, 128, 3) and one.dtype == torch.uint8 and one.is_cuda
    both = flow_viz.omniflow_to_image(flow)
    assert tuple(both.shape) == (2, 64, 128, 3) and torch.equal(both[0], one)             # every image has its own clip
    assert torch.equal(flow_viz.omniflow_to_image(flow[0], convert_to_bgr=True), one.flip(-1))
    ck.colour_figures(both.cpu().numpy(), gold["omni_64x128"], "omniflow_to_image 64x128")
    ck.colour_figures(flow_viz.flow_to_image(flow).cpu().numpy(), gold["plane_64x128"], "flow_to_image 64x128")
    img = torch.from_numpy(gold["image_64x128"].astype(np.float32)).cuda()
    w = flow_viz.my_cycle_warp(img, flow[:1])
    assert np.abs(w.cpu().numpy() - gold["warp_64x128"]).max() <= ck.WARP_ATOL
    with pytest.raises(PfError):
        flow_viz.omniflow_to_image(flow[0], clip_flow=5.0)
    with pytest.raises(PfError):
        flow_viz.omniflow_to_image(flow[0].cpu())
    with pytest.raises(PfError):
        flow_viz.my_cycle_warp(img.cpu(), flow[:1])


@pytest.mark.parametrize("mode,layout", [("omni", "hwc"), ("plane", "chw")])
def test_renderer_captured_equals_eager_and_allocates_nothing(lib, mode, layout):
    from prior_flow_amd.flow_viz import FlowRenderer
    B, H, W = 2, 128, 256
    flows = [torch.from_numpy(fc.make_flow(B, H, W, seed=s)).cuda() for s in (41, 42, 43)]
    im1 = [torch.from_numpy(fc.make_image(B, 3, H, W, seed=s)).cuda() for s in (41, 42, 43)]
    im2 = [torch.from_numpy(fc.make_image(B, 3, H, W, seed=s + 10)).cuda() for s in (41, 42, 43)]
    occs = [(torch.rand(B, H, W, device="cuda") < 0.2).to(torch.uint8) for _ in range(3)]
    eager = FlowRenderer(B, H, W, "cuda", mode=mode, layout=layout)
    eager.prepare_warp(3)
    want = []
    for f, a, b, o in zip(flows, im1, im2, occs):
        rgb = eager.render(f).clone()
        wp, err, mean = eager.warp(b, f, image1=a, occ=o)
        want.append((rgb, wp.clone(), err.clone(), mean.clone()))
    r = FlowRenderer(B, H, W, "cuda", mode=mode, layout=layout)
    r.prepare_warp(3)
    f_in, a_in, b_in, o_in = torch.zeros_like(flows[0]), torch.zeros_like(im1[0]), torch.zeros_like(im2[0]), torch.zeros_like(occs[0])
    r.render(f_in)
    r.warp(b_in, f_in, image1=a_in, occ=o_in)           # warm-up outside the capture
    torch.cuda.synchronize()
    before, n_before = torch.cuda.memory_allocated(), torch.cuda.memory_stats()["allocation.all.allocated"]
    for _ in range(3):
        r.render(f_in)
        r.warp(b_in, f_in, image1=a_in, occ=o_in)
    assert torch.cuda.memory_allocated() == before      # construction, then no allocation
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == n_before
    # inside the capture, around the renderer's calls alone (what beginning and ending a capture allocates for itself -- the
    # generator state a graph registers -- is not the renderer's): the allocator's event count does not move
    events = lambda: torch.cuda.memory_stats()["allocation.all.allocated"]      # noqa: E731
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        n0 = events()
        rgb = r.render(f_in)
        wp, err, mean = r.warp(b_in, f_in, image1=a_in, occ=o_in)
        n1 = events()
    assert n1 == n0, (n0, n1)
    for i in (1, 2, 0):                                  # new flows in the same buffers
        f_in.copy_(flows[i]); a_in.copy_(im1[i]); b_in.copy_(im2[i]); o_in.copy_(occs[i])
        g.replay()
        torch.cuda.synchronize()
        for got, w in zip((rgb, wp, err, mean), want[i]):
            assert torch.equal(got, w)
    m = want[0][3].cpu().numpy()
    ref_mean = fr.photometric(im1[0].cpu().numpy(), want[0][1].cpu().numpy(), occs[0].cpu().numpy())[1]
    assert np.allclose(m, ref_mean, rtol=ck.MEAN_ERR_RTOL, atol=0)


# ---- composition with the stream and the demo --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    from prior_flow_amd.modules import state_dict_shapes
    from prior_flow_amd.prior_raft import PriOr_RAFT
    m = PriOr_RAFT(argparse.Namespace(mixed_precision=False, dropout=0.0, alternate_corr=False))
    m.load_state_dict(gc.det_state_dict(state_dict_shapes()), strict=True)
    return m.cuda().eval()


def test_stream_then_render(model):
    from prior_flow_amd.flow_viz import FlowRenderer
    from prior_flow_amd.video import FlowStream
    B, H, W, iters = 1, 128, 256, 4
    f0, _ = gc.synthetic_pair(B, H, W, seed=5)
    frames = [torch.roll(f0, shifts=(t, 3 * t), dims=(2, 3)).cuda() for t in range(3)]
    r = FlowRenderer(B, H, W, "cuda")
    with torch.no_grad():
        s = FlowStream(model, iters=iters, warm_start=False)
        assert s(frames[0]) is None
        for t in (1, 2):
            flow = s(frames[t])
            got = r.render(flow).clone()
            pair = model(frames[t - 1], frames[t], iters=iters, test_mode=True)
            same = torch.equal(flow, pair)
            want = r.render(pair.contiguous()).clone()
            print(f"[flow_viz] stream pair {t}: flow equal to the per-pair call bit for bit: {same}; "
                  f"differing bytes {int((got != want).sum())}")
            assert torch.equal(got, want)


def test_demo_image_writes_the_rendered_flow(model, tmp_path):
    from PIL import Image
    from prior_flow_amd import demo_image, flow_viz
    i1, i2 = gc.synthetic_pair(1, 128, 256, seed=7)
    to_u8 = lambda t: t[0].permute(1, 2, 0).clamp(0, 255).to(torch.uint8).numpy()      # noqa: E731
    p1, p2, out = (str(tmp_path / n) for n in ("a.png", "b.png", "flow_pr.png"))
    Image.fromarray(to_u8(i1)).save(p1)
    Image.fromarray(to_u8(i2)).save(p2)
    args = demo_image.parse_args(["--img1", p1, "--img2", p2, "--out", out, "--iters", "4"])
    demo_image.run(args)                                 # the command line's path: no --model, det_state_dict weights (the fixture's)
    with torch.no_grad():
        flow = model(demo_image.load_image(p1), demo_image.load_image(p2), iters=4, test_mode=True)
    want = flow_viz.omniflow_to_image(flow[0]).cpu().numpy()
    assert os.path.getsize(out) > 0
    assert np.array_equal(np.array(Image.open(out)), want)
