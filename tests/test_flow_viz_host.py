"""Flow rendering without a GPU: the host emulation of pf_order_stat / pf_flow_render / pf_cycle_warp /
pf_masked_mean (csrc/pf_elem.h + pf_api_elem.inc) against np.sort, the reference's results in tests/golden/flow_viz.npz and the
float64 restatement of tests/flow_viz_ref.py; hand cases; the argument checks of the entry points before any launch.

Measured (host emulation against the reference's bytes, share of differing values, never by more than 1; bar 0.5 %):
omni 0 / 1.0e-5 / 0 and plane 0 / 2.0e-5 / 0 at 64x128 / 128x256 / 136x216; length map against calculate_veclen_spherical
3.0e-8 - 1.2e-7 (bar 2e-6); warp against the reference's my_cycle_warp at the three sizes (W = 216 included, where the fp32 `% W`
of torch and pf_pymod could differ): 0 (bit for bit; bar 2e-4); the restatement's warp against it: 3.1e-5 - 3.2e-5."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import flow_viz_cases as fc
import flow_viz_checks as ck
import flow_viz_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
EMU_SO = os.path.join(EMU_DIR, "libpf_emu.so")
CSRC = os.path.join(ROOT, "prior-flow_amd", "csrc")


@pytest.fixture(scope="module")
def emu():
    import emu_lib
    return emu_lib.load()


@pytest.fixture(scope="module")
def gold():
    return ck.golden()


# ---- the order statistic ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", [29376, 1000003])
@pytest.mark.parametrize("kind", ck.OS_KINDS)
def test_order_stat_is_np_sort_bit_for_bit(emu, kind, n, B):
    x = ck.os_input(kind, B, n, seed=n % 97 + B)
    for k in ck.os_ranks(n):
        got = ck.run_order_stat(emu, x, k)
        want = ck.os_expected(x, k)
        assert got.view(np.uint32).tolist() == want.view(np.uint32).tolist(), (kind, n, B, k, got, want)


def test_order_stat_nan_rules(emu):
    """NaN ranks last; a rank that falls on a NaN gives the largest value that is not NaN, 0 when there is none."""
    x = np.array([[3.0, np.nan, 1.0, np.nan, 2.0], [np.nan] * 5, [0.5, np.inf, np.nan, 0.25, 0.0]], np.float32)
    assert ck.run_order_stat(emu, x, 2).tolist() == [3.0, 0.0, 0.5]
    assert ck.run_order_stat(emu, x, 3).tolist() == [3.0, 0.0, np.inf]
    assert ck.run_order_stat(emu, x, 4).tolist() == [3.0, 0.0, np.inf]
    assert ck.run_order_stat(emu, x, 0).tolist() == [1.0, 0.0, 0.0]


def test_order_stat_tiny_and_denormal(emu):
    x = np.array([[1e-45, 0.0, 1e-38, 3e-39, 1e-45, 1.0]], np.float32)
    for k in range(6):
        assert ck.run_order_stat(emu, x, k).view(np.uint32)[0] == np.sort(x[0])[k].view(np.uint32)


# ---- the restatement against the reference's stored results ------------------------------------------------------------------
@pytest.mark.parametrize("H,W", fc.SIZES)
def test_restatement_matches_the_reference(gold, H, W):
    flow = ck.fixture_flow(gold, H, W)
    assert np.array_equal(fc.make_flow(fc.FIXTURE_BATCH[(H, W)], H, W, seed=10 + fc.SIZES.index((H, W))), flow)   # the stored inputs are the cases
    sd = fr.veclen_spherical(flow)
    assert np.abs(sd - gold[f"sd_{H}x{W}"]).max() <= ck.SD_ATOL
    ck.colour_figures(fr.render(flow, "omni"), gold[f"omni_{H}x{W}"], f"restatement omni {H}x{W}")
    ck.colour_figures(fr.render(flow, "plane"), gold[f"plane_{H}x{W}"], f"restatement plane {H}x{W}")
    assert np.array_equal(fr.colorwheel().shape, (55, 3))
    img = gold[f"image_{H}x{W}"].astype(np.float32)
    assert img.shape[1] == fc.FIXTURE_WARP[(H, W)]
    d = np.abs(fr.cycle_warp(img, flow[:1]) - gold[f"warp_{H}x{W}"]).max()
    print(f"[flow_viz] restatement warp against my_cycle_warp {H}x{W}: {d:.3e}")
    assert d <= ck.WARP_ATOL


# ---- render ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", fc.SIZES)
def test_render_matches_the_reference(emu, gold, H, W):
    flow = ck.fixture_flow(gold, H, W)
    img, length, clip = ck.run_render(emu, flow, "omni")
    d = np.abs(length.astype(np.float64) - gold[f"sd_{H}x{W}"]).max()
    print(f"[flow_viz] emulation len against calculate_veclen_spherical {H}x{W}: {d:.3e}")
    assert d <= ck.SD_ATOL
    # the clip is the exact order statistic of the emulation's own length map, and it is the reference's up to the same bar
    want_clip = np.array([np.sort(length[b], axis=None)[int(0.95 * H * W)] for b in range(len(flow))])
    assert clip.view(np.uint32).tolist() == want_clip.astype(np.float32).view(np.uint32).tolist()
    assert np.abs(clip - gold[f"clip_{H}x{W}"]).max() <= ck.SD_ATOL
    ck.colour_figures(img, gold[f"omni_{H}x{W}"], f"emulation omni {H}x{W}")
    ck.colour_figures(img, fr.render(flow, "omni"), f"emulation omni {H}x{W} against float64")
    imgp, lenp, clipp = ck.run_render(emu, flow, "plane")
    assert clipp.view(np.uint32).tolist() == lenp.reshape(len(flow), -1).max(1).view(np.uint32).tolist()
    ck.colour_figures(imgp, gold[f"plane_{H}x{W}"], f"emulation plane {H}x{W}")


def test_render_layouts_and_bgr(emu, gold):
    flow = ck.fixture_flow(gold, 64, 128)
    rgb = ck.run_render(emu, flow, "omni")[0]
    assert np.array_equal(ck.run_render(emu, flow, "omni", bgr=True)[0], rgb[..., ::-1])
    assert np.array_equal(ck.run_render(emu, flow, "omni", layout="chw")[0], rgb.transpose(0, 3, 1, 2))
    assert np.array_equal(ck.run_render(emu, flow, "omni", layout="chw", bgr=True)[0], rgb[..., ::-1].transpose(0, 3, 1, 2))
    ck.colour_figures(ck.run_render(emu, flow[:1], "omni", bgr=True)[0], gold["omni_bgr_64x128"], "emulation omni bgr 64x128")


def test_render_other_percentiles(emu, gold):
    flow = ck.fixture_flow(gold, 64, 128)
    for p in (0.0, 0.5, 1.0):
        img, length, clip = ck.run_render(emu, flow, "omni", percentile=p)
        k = min(int(p * 64 * 128), 64 * 128 - 1)
        assert clip.tolist() == [np.sort(length[b], axis=None)[k] for b in range(2)]
        ck.colour_figures(img, fr.render(flow, "omni", percentile=p), f"emulation omni percentile {p}")


def test_antipodal_flow_is_finite_and_ranked(emu):
    """Finite flows to the far side of the sphere (half a turn next to the equator, pole row to pole row): the haversine comes
    within rounding of 1, which pf_render_len clamps; the length stays finite, the pixel is ranked and coloured, not black."""
    H, W = 64, 128
    flow = np.zeros((1, 2, H, W), np.float32)
    flow[0, 0, H // 2 - 1:H // 2 + 1] = W / 2            # the two rows next to the equator
    flow[0, 1, 0] = H                                     # from the top row past the bottom one (y clamps)
    flow[0, 0, 0] = W / 2
    img, length, clip = ck.run_render(emu, flow, "omni", percentile=1.0)
    assert np.isfinite(length).all() and np.isfinite(clip).all()
    assert abs(float(length.max()) - (np.pi - np.pi / (2 * H))) <= 1e-5      # top row centre -> bottom edge, half a turn away
    assert abs(float(length[0, H // 2, 0]) - (np.pi - np.pi / H)) <= 1e-5     # half a pixel off the equator, half a turn
    assert (img.reshape(-1, 3).max(1) > 0).all()


def test_zero_flow_is_white(emu):
    for mode in ("omni", "plane"):
        img = ck.run_render(emu, np.zeros((2, 2, 16, 32), np.float32), mode)[0]
        assert (img == 255).all()


def test_non_finite_pixel_is_black_and_alone(emu, gold):
    flow = ck.fixture_flow(gold, 64, 128)
    bad = flow.copy()
    spots = [(0, 0, 5, 7, np.nan), (0, 1, 20, 100, np.inf), (1, 0, 63, 127, -np.inf), (1, 1, 30, 0, np.nan)]
    for b, c, y, x, v in spots:
        bad[b, c, y, x] = v
    img, length, clip = ck.run_render(emu, bad, "omni")
    for b, c, y, x, v in spots:
        assert img[b, y, x].tolist() == [0, 0, 0]
        assert np.isnan(length[b, y, x])
    assert np.isnan(length).sum() == len(spots) and (img.reshape(-1, 3).max(1) == 0).sum() == len(spots)     # nothing else is touched
    # the pixels that left the ranks move the clip to a neighbouring value; the rest of the image follows the restatement, which
    # ranks them last as well
    ck.colour_figures(img, fr.render(bad, "omni"), "non-finite, omni")
    imgp = ck.run_render(emu, bad, "plane")[0]
    for b, c, y, x, v in spots:
        assert imgp[b, y, x].tolist() == [0, 0, 0]
    assert (imgp.reshape(-1, 3).max(1) == 0).sum() == len(spots)
    ck.colour_figures(imgp, fr.render(bad, "plane"), "non-finite, plane")
    # the neighbours bit for bit: with the clip pinned (percentile 0: the smallest length, 0 in the region at rest, in both runs)
    a = ck.run_render(emu, flow, "omni", percentile=0.0)[0]
    b_ = ck.run_render(emu, bad, "omni", percentile=0.0)[0]
    keep = np.ones((2, 64, 128), bool)
    for b, c, y, x, v in spots:
        keep[b, y, x] = False
    assert np.array_equal(a[keep], b_[keep])


# ---- warp ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,C", ck.WARP_CASES)
def test_warp_matches_the_reference(emu, gold, H, W, C):
    flow = ck.fixture_flow(gold, H, W)[:1]
    img = gold[f"image_{H}x{W}"].astype(np.float32)[:, :C].copy()
    got, _ = ck.run_warp(emu, img, flow)
    d = np.abs(got.astype(np.float64) - gold[f"warp_{H}x{W}"][:, :C]).max()
    print(f"[flow_viz] emulation warp C={C} against my_cycle_warp {H}x{W}: {d:.3e}")
    assert d <= ck.WARP_ATOL


@pytest.mark.parametrize("C", [1, 3, 5])
@pytest.mark.parametrize("H,W", [(64, 128), (136, 216), (64, 130)])
def test_warp_matches_float64(emu, H, W, C):
    flow = fc.make_flow(2, H, W, seed=5)
    img = fc.make_image(2, C, H, W, seed=5)
    ref = fc.make_image(2, C, H, W, seed=6)
    got, err = ck.run_warp(emu, img, flow, ref=ref)
    assert np.abs(got - fr.cycle_warp(img, flow)).max() <= ck.WARP_ATOL
    want_err, _ = fr.photometric(ref, got)
    assert np.abs(err - want_err).max() <= 255 * 2.0 ** -22          # mean of C fp32 absolute differences
    alone, none = ck.run_warp(emu, img, flow)
    assert none is None and np.array_equal(alone, got)


def test_integer_pan_is_a_roll(emu):
    x = fc.make_image(2, 3, 16, 32, seed=3)
    for k in (5, -3, 32 + 7):
        pan = np.zeros((2, 2, 16, 32), np.float32)
        pan[:, 0] = k
        assert np.array_equal(ck.run_warp(emu, x, pan)[0], np.roll(x, -k, axis=3))
    down = np.zeros((2, 2, 16, 32), np.float32)
    down[:, 1] = 2
    want = np.concatenate([x[:, :, 2:], x[:, :, -1:], x[:, :, -1:]], axis=2)      # y clamps
    assert np.array_equal(ck.run_warp(emu, x, down)[0], want)


def test_masked_mean(emu):
    rng = np.random.default_rng(4)
    for B, N in ((1, 100), (3, 64 * 130), (2, 300001)):
        x = np.abs(rng.standard_normal((B, N))).astype(np.float32) * 20
        occ = (rng.random((B, N)) < 0.3).astype(np.uint8)
        occ[-1] = 1                                                  # every pixel occluded -> 0
        got = ck.run_masked_mean(emu, x, occ)
        want = np.array([x[b][occ[b] == 0].astype(np.float64).mean() if (occ[b] == 0).any() else 0.0 for b in range(B)])
        assert np.allclose(got, want, rtol=ck.MEAN_ERR_RTOL, atol=0), (got, want)
        assert got[-1] == 0.0
        assert np.allclose(ck.run_masked_mean(emu, x, None), x.astype(np.float64).mean(1), rtol=ck.MEAN_ERR_RTOL, atol=0)


# ---- refusals before any launch ----------------------------------------------------------------------------------------------
def test_argument_refusals(emu):
    dll = emu._dll
    BAD_ARG, BAD_SHAPE = -1, -2
    f = np.zeros((1, 2, 8, 16), np.float32)
    img = np.zeros((1, 8, 16, 3), np.uint8)
    sc = np.zeros(int(dll.pf_flow_render_scratch_bytes(1, 8, 16)) // 4 + 1, np.int32)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    nb = sc.nbytes
    assert dll.pf_flow_render(P(f), P(img), P(sc), nb, 1, 8, 16, 0, 0.95, 0, 0, None) == 0
    assert dll.pf_flow_render(None, P(img), P(sc), nb, 1, 8, 16, 0, 0.95, 0, 0, None) == BAD_ARG
    assert dll.pf_flow_render(P(f), None, P(sc), nb, 1, 8, 16, 0, 0.95, 0, 0, None) == BAD_ARG
    assert dll.pf_flow_render(P(f), P(img), None, nb, 1, 8, 16, 0, 0.95, 0, 0, None) == BAD_ARG
    assert dll.pf_flow_render(P(f), P(img), P(sc), nb, 1, 8, 16, 2, 0.95, 0, 0, None) == BAD_ARG        # mode
    assert dll.pf_flow_render(P(f), P(img), P(sc), nb, 1, 8, 16, 0, 0.95, 2, 0, None) == BAD_ARG        # layout
    assert dll.pf_flow_render(P(f), P(img), P(sc), nb, 1, 8, 16, 0, 0.95, 0, 3, None) == BAD_ARG        # bgr
    assert dll.pf_flow_render(P(f), P(img), P(sc), nb, 1, 8, 16, 0, 1.5, 0, 0, None) == BAD_ARG
    assert dll.pf_flow_render(P(f), P(img), P(sc), nb, 1, 8, 16, 0, float("nan"), 0, 0, None) == BAD_ARG
    assert dll.pf_flow_render(P(f), P(img), P(sc), 100, 1, 8, 16, 0, 0.95, 0, 0, None) == BAD_ARG       # short scratch
    assert dll.pf_flow_render(P(f), P(img), P(sc), nb, 0, 8, 16, 0, 0.95, 0, 0, None) == BAD_SHAPE
    assert dll.pf_flow_render(P(f), P(img), P(sc), nb, 1, 1, 16, 0, 0.95, 0, 0, None) == BAD_SHAPE
    assert dll.pf_flow_render(P(f), P(img), P(sc), nb, 65536, 8, 16, 0, 0.95, 0, 0, None) == BAD_SHAPE    # more images than grid rows
    assert dll.pf_flow_render_scratch_bytes(0, 8, 16) == BAD_SHAPE
    assert dll.pf_flow_render_scratch_bytes(65536, 8, 16) == BAD_SHAPE
    x = np.ones(64, np.float32)
    out = np.zeros(1, np.float32)
    so = np.zeros(int(dll.pf_order_stat_scratch_bytes(1, 64)) // 4, np.int32)
    assert dll.pf_order_stat(P(x), P(out), P(so), so.nbytes, 1, 64, 63, None) == 0
    assert dll.pf_order_stat(P(x), P(out), P(so), so.nbytes, 1, 64, 64, None) == BAD_ARG                # k >= n
    assert dll.pf_order_stat(P(x), P(out), P(so), so.nbytes, 1, 64, -1, None) == BAD_ARG
    assert dll.pf_order_stat(P(x), P(out), P(so), so.nbytes - 4, 1, 64, 0, None) == BAD_ARG
    assert dll.pf_order_stat(P(x), P(x), P(so), so.nbytes, 1, 64, 0, None) == BAD_ARG
    assert dll.pf_order_stat(None, P(out), P(so), so.nbytes, 1, 64, 0, None) == BAD_ARG
    assert dll.pf_order_stat(P(x), P(out), P(so), so.nbytes, 0, 64, 0, None) == BAD_SHAPE
    assert dll.pf_order_stat(P(x), P(out), P(so), so.nbytes, 1, 0, 0, None) == BAD_SHAPE
    assert dll.pf_order_stat(P(x), P(out), P(so), 1 << 40, 65536, 64, 0, None) == BAD_SHAPE
    assert dll.pf_order_stat_scratch_bytes(1, 0) == BAD_SHAPE
    assert dll.pf_order_stat_scratch_bytes(65536, 64) == BAD_SHAPE
    a = np.zeros((1, 3, 8, 16), np.float32)
    o = np.zeros_like(a)
    e = np.zeros((1, 8, 16), np.float32)
    assert dll.pf_cycle_warp(P(a), P(f), None, P(o), None, 1, 3, 8, 16, None) == 0
    assert dll.pf_cycle_warp(P(a), P(f), None, P(a), None, 1, 3, 8, 16, None) == BAD_ARG               # in place
    assert dll.pf_cycle_warp(P(a), P(f), P(a), P(o), None, 1, 3, 8, 16, None) == BAD_ARG               # ref without err
    assert dll.pf_cycle_warp(P(a), P(f), None, P(o), P(e), 1, 3, 8, 16, None) == BAD_ARG               # err without ref
    assert dll.pf_cycle_warp(None, P(f), None, P(o), None, 1, 3, 8, 16, None) == BAD_ARG
    assert dll.pf_cycle_warp(P(a), P(f), None, P(o), None, 1, 0, 8, 16, None) == BAD_SHAPE
    assert dll.pf_cycle_warp(P(a), P(f), None, P(o), None, 1, 3, 8, 1, None) == BAD_SHAPE
    sm = np.zeros(128, np.float64)
    assert dll.pf_masked_mean(P(e), None, P(out), P(sm), sm.nbytes, 1, 128, None) == 0
    assert dll.pf_masked_mean(P(e), None, P(out), P(sm), 512, 1, 128, None) == BAD_ARG
    assert dll.pf_masked_mean(P(e), None, P(out), P(sm), sm.nbytes, 1, 0, None) == BAD_SHAPE
    assert dll.pf_masked_mean(P(e), None, P(out), P(sm), 1 << 40, 65536, 128, None) == BAD_SHAPE
    assert dll.pf_masked_mean(P(e), None, P(out), P(sm), sm.nbytes, 1, 1 << 30, None) == BAD_SHAPE


def test_binding_refusals(emu):
    from prior_flow_amd._lib import PfError
    f = torch.zeros(1, 2, 8, 16)
    sc = torch.zeros(emu.flow_render_scratch_bytes(1, 8, 16) // 4 + 1, dtype=torch.int32)
    with pytest.raises(PfError):
        emu.flow_render(f.double(), torch.zeros(1, 8, 16, 3, dtype=torch.uint8), sc)
    with pytest.raises(PfError):
        emu.flow_render(f, torch.zeros(1, 8, 16, 3, dtype=torch.float32), sc)
    with pytest.raises(PfError):
        emu.flow_render(f, torch.zeros(1, 3, 8, 16, dtype=torch.uint8), sc)                 # shape of the other layout
    with pytest.raises(PfError):
        emu.flow_render(f, torch.zeros(1, 8, 16, 3, dtype=torch.uint8), sc, mode="sphere")
    with pytest.raises(PfError):
        emu.flow_render(f[:, :1], torch.zeros(1, 8, 16, 3, dtype=torch.uint8), sc)
    with pytest.raises(PfError):
        emu.cycle_warp(torch.zeros(1, 3, 8, 16), f, torch.zeros(1, 3, 8, 16), ref=torch.zeros(1, 3, 8, 16))


def test_python_interface_refuses_cpu_tensors_and_clip_flow():
    from prior_flow_amd import flow_viz
    from prior_flow_amd._lib import PfError
    f = torch.zeros(2, 8, 16)
    for fn in (flow_viz.omniflow_to_image, flow_viz.flow_to_image):
        with pytest.raises(PfError):
            fn(f)
    with pytest.raises(PfError):
        flow_viz.my_cycle_warp(torch.zeros(1, 3, 8, 16), torch.zeros(1, 2, 8, 16))
    with pytest.raises(PfError):
        flow_viz.FlowRenderer(1, 8, 16, "cpu")
    with pytest.raises(PfError):
        flow_viz._to_image(f, 10.0, False, "omni", "omniflow_to_image")
