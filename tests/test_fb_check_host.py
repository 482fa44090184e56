"""The forward-backward check without a GPU: the host emulation of pf_fb_check's element form (csrc/pf_elem.h) against the
float64 restatement of tests/fb_check_ref.py -- constructed flows (smooth, across the seam, past the poles), hand cases, and
the argument checks of the entry point before any launch."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import fb_check_ref as fb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
EMU_SO = os.path.join(EMU_DIR, "libpf_emu.so")
CSRC = os.path.join(ROOT, "prior-flow_amd", "csrc")


@pytest.fixture(scope="module")
def emu():
    import emu_lib
    return emu_lib.load()


def run(lib, fw: np.ndarray, bw: np.ndarray, metric: str, alpha=0.01, beta=0.5, device=None):
    """pf_fb_check through the binding on [B,2,H,W] float32 arrays -> numpy (occ_fw, occ_bw, res_fw, res_bw)."""
    f, b = torch.from_numpy(np.ascontiguousarray(fw)), torch.from_numpy(np.ascontiguousarray(bw))
    if device is not None:
        f, b = f.to(device), b.to(device)
    B, _, H, W = f.shape
    occ = [torch.full((B, H, W), 7, dtype=torch.uint8, device=f.device) for _ in range(2)]
    res = [torch.full_like(f, float("nan")) for _ in range(2)]
    lib.fb_check(f, b, occ[0], occ[1], res[0], res[1], metric=metric, alpha=alpha, beta=beta)
    return tuple(t.cpu().numpy() for t in occ + res)


def check_case(lib, kind, H, W, metric, device=None):
    """B = 2, both directions, against the float64 restatement; returns the figures of the four (image, direction) cases."""
    fw, bw = fb.batch(kind, H, W)
    occ_fw, occ_bw, res_fw, res_bw = run(lib, fw, bw, metric, device=device)
    figures = []
    for b in range(2):
        figures.append(fb.check(occ_fw[b], res_fw[b], fb.reference(fw[b], bw[b], metric), f"{kind} {H}x{W} {metric} image {b} forward"))
        figures.append(fb.check(occ_bw[b], res_bw[b], fb.reference(bw[b], fw[b], metric), f"{kind} {H}x{W} {metric} image {b} backward"))
    return figures


@pytest.mark.parametrize("metric", ["plane", "sphere"])
@pytest.mark.parametrize("H,W", [(64, 128), (128, 256)])
@pytest.mark.parametrize("kind", fb.KINDS)
def test_emulated_fb_check_matches_float64(emu, kind, H, W, metric):
    figures = check_case(emu, kind, H, W, metric)
    assert all(0.0 < f["occluded"] < 1.0 for f in figures)          # both outcomes are exercised


def test_reference_flags_what_it_should():
    """The restatement itself: a consistent pair passes everywhere, the block that disagrees is flagged."""
    fw, bw = fb.pair("smooth", 64, 128, 3)
    for metric in ("plane", "sphere"):
        ref = fb.reference(fw, bw, metric)
        # where the forward flow lands in the disagreeing block (rows H/4..H/2, columns W/8..W/3) the round trip is off by ~(7, -5)
        y, x = np.mgrid[0:64, 0:128]
        qx, qy = np.mod(x + fw[0], 128), y + fw[1]
        inside = (qy > 18) & (qy < 30) & (qx > 18) & (qx < 40)
        assert ref["occ"][inside].all() and ref["occ"].mean() < 0.6


@pytest.mark.parametrize("metric", ["plane", "sphere"])
def test_hand_cases(emu, metric):
    H, W = 32, 64
    zero = np.zeros((1, 2, H, W), np.float32)
    occ_fw, occ_bw, res_fw, res_bw = run(emu, zero, zero.copy(), metric)
    assert not occ_fw.any() and not occ_bw.any() and not res_fw.any() and not res_bw.any()
    for k in (3, W // 2 - 1):           # a pure cyclic pan: consistent everywhere, across the seam and at +-W/2 included
        fw, bw = zero.copy(), zero.copy()
        fw[:, 0] = k
        bw[:, 0] = -k
        occ_fw, occ_bw, res_fw, res_bw = run(emu, fw, bw, metric)
        assert not occ_fw.any() and not occ_bw.any(), k
        assert not res_fw.any() and not res_bw.any(), k
    # NaN / Inf in: occluded, residual 0 -- at the pixel itself (forward) and where a tap of the sample reads it (backward)
    fw, bw = zero.copy(), zero.copy()
    fw[0, 0, 5, 7] = np.nan
    fw[0, 1, 9, 11] = np.inf
    occ_fw, occ_bw, res_fw, res_bw = run(emu, fw, bw, metric)
    assert occ_fw[0, 5, 7] == 1 and occ_fw[0, 9, 11] == 1 and occ_fw.sum() == 2
    assert occ_bw[0, 5, 7] == 1 and occ_bw[0, 9, 11] == 1
    assert np.isfinite(res_fw).all() and np.isfinite(res_bw).all() and res_fw[0, :, 5, 7].tolist() == [0.0, 0.0]
    # a flow that disagrees by more than the threshold in one spot
    fw, bw = zero.copy(), zero.copy()
    fw[0, 0, 10, 10] = 2.0
    occ_fw, _, res_fw, _ = run(emu, fw, bw, metric)
    assert occ_fw[0, 10, 10] == 1 and occ_fw.sum() == 1 and res_fw[0, 0, 10, 10] == 2.0


def test_sphere_threshold_is_an_angle():
    """The same half-pixel disagreement passes nowhere on the plane; on the sphere a horizontal disagreement of 2 px is a
    failure at the equator and, next to a pole, too small an angle to count."""
    H, W = 64, 128
    fw = np.zeros((2, H, W), np.float32)
    bw = np.zeros((2, H, W), np.float32)
    bw[0] = 2.0
    plane, sphere = fb.reference(fw, bw, "plane"), fb.reference(fw, bw, "sphere")
    assert plane["occ"].all()
    assert sphere["occ"][H // 2].all() and not sphere["occ"][0].any() and not sphere["occ"][H - 1].any()


def test_entry_point_refuses_bad_arguments(emu):
    """PF_ERR_* before any launch, in the emulation build (and the device build when it has been built)."""
    libs = [ctypes.CDLL(EMU_SO)]
    from prior_flow_amd import _lib
    if os.path.exists(_lib.LIB_PATH):
        libs.append(ctypes.CDLL(_lib.LIB_PATH))
    H, W = 4, 8
    bufs = [(ctypes.c_float * (2 * H * W))() for _ in range(6)]
    fw, bw, of, ob, rf, rb = [ctypes.cast(b, ctypes.c_void_p) for b in bufs]
    for dll in libs:
        fn = dll.pf_fb_check
        fn.argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_int] * 4 + [ctypes.c_float] * 2 + [ctypes.c_void_p]
        fn.restype = ctypes.c_int
        ok = (fw, bw, of, ob, rf, rb, 1, H, W, 1, 0.01, 0.5, None)
        for i in range(6):                                                  # a NULL pointer
            assert fn(*(ok[:i] + (None,) + ok[i + 1:])) == -1, i
        assert fn(fw, fw, of, ob, rf, rb, 1, H, W, 1, 0.01, 0.5, None) == -1        # one flow given twice
        assert fn(fw, bw, of, ob, fw, rb, 1, H, W, 1, 0.01, 0.5, None) == -1        # a residual over its input
        assert fn(fw, bw, of, ob, rf, rf, 1, H, W, 1, 0.01, 0.5, None) == -1        # both residuals in one buffer
        assert fn(fw, bw, of, of, rf, rb, 1, H, W, 1, 0.01, 0.5, None) == -1        # both masks in one buffer
        assert fn(fw, bw, of, ob, rf, rb, 1, H, W, 2, 0.01, 0.5, None) == -1        # unknown metric
        assert fn(fw, bw, of, ob, rf, rb, 1, H, W, 0, -0.01, 0.5, None) == -1       # negative alpha
        assert fn(fw, bw, of, ob, rf, rb, 1, H, W, 0, 0.01, float("nan"), None) == -1
        assert fn(fw, bw, of, ob, rf, rb, 0, H, W, 1, 0.01, 0.5, None) == -2        # empty batch
        assert fn(fw, bw, of, ob, rf, rb, 1, 1, W, 1, 0.01, 0.5, None) == -2        # one row
        assert fn(fw, bw, of, ob, rf, rb, 1, 1 << 15, 1 << 15, 1, 0.01, 0.5, None) == -2
    from prior_flow_amd._lib import PfError
    f = torch.zeros(1, 2, H, W)
    occ, res = torch.zeros(1, H, W, dtype=torch.uint8), torch.zeros(1, 2, H, W)
    with pytest.raises(PfError):
        emu.fb_check(f, f.clone(), occ, occ.clone(), res, res.clone(), metric="cube")
    with pytest.raises(PfError):
        emu.fb_check(f, torch.zeros(1, 2, H, W + 1), occ, occ.clone(), res, res.clone())
    with pytest.raises(PfError):
        emu.fb_check(f, f.clone(), occ.float(), occ.clone(), res, res.clone())


def test_python_check_and_stream_arguments_need_a_device():
    """forward_backward_check has no CPU path; the stream knows its new arguments and refuses an unknown metric."""
    from prior_flow_amd import video
    from prior_flow_amd._lib import PfError
    with pytest.raises(PfError):
        video.forward_backward_check(torch.zeros(1, 2, 16, 32), torch.zeros(1, 2, 16, 32))
    s = video.FlowStream(None, iters=2, bidirectional=True, occlusion="plane")
    assert s.bidirectional and s.occlusion == "plane" and s.flow_low_backward is None
    with pytest.raises(PfError):
        video.FlowStream(None, bidirectional=True, occlusion="cube")
    with pytest.raises(PfError):
        video.FlowStream(None, bidirectional=False, occlusion="sphere")
    assert video.BidirectionalFlow._fields == ("forward", "backward", "occ_forward", "occ_backward", "residual_forward", "residual_backward")
