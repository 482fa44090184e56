"""forward_interpolate and the single-frame input stage without a GPU: the float64 brute force of the tests
(tests/fwd_interp_ref.py) against the reference's scipy griddata, the host emulation of the kernel's element forms
(csrc/pf_elem.h: pf_fi_*) against that brute force, and the argument checks of the new entry points before any launch."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import fwd_interp_ref as fref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
EMU_SO = os.path.join(EMU_DIR, "libpf_emu.so")
CSRC = os.path.join(ROOT, "prior-flow_amd", "csrc")
NEW = ("pf_forward_interpolate", "pf_prepare_frame")


@pytest.fixture(scope="module")
def emu():
    import emu_lib
    return emu_lib.load()


def flows(kind: str, h: int, w: int, seed: int = 0) -> np.ndarray:
    """[2,h,w] float32 test fields: smooth, large displacements (holes and pile-ups), points leaving the frame, all invalid."""
    g = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    if kind == "smooth":
        u = 3.0 * np.sin(x / w * 2 * np.pi + 0.3) + g.normal(0, 0.2, (h, w))
        v = 2.0 * np.cos(y / h * np.pi) + g.normal(0, 0.2, (h, w))
    elif kind == "large":
        u = np.where(x < w / 2, 0.4 * w, -0.1 * w) + g.normal(0, 1.5, (h, w))
        v = np.where(y < h / 2, 0.25 * h, -0.05 * h) + g.normal(0, 1.5, (h, w))
    elif kind == "leaving":
        u = (x - w / 2) * 0.8 + g.normal(0, 0.5, (h, w))
        v = (y - h / 2) * 0.8 + g.normal(0, 0.5, (h, w))
    elif kind == "integer":                 # whole-pixel moves: exact ties between points at equal distances
        u = g.integers(-3, 4, (h, w)).astype(np.float64)
        v = g.integers(-2, 3, (h, w)).astype(np.float64)
    elif kind == "invalid":
        u = np.full((h, w), 2.0 * w)
        v = np.full((h, w), -2.0 * h)
    else:
        raise ValueError(kind)
    return np.stack([u, v]).astype(np.float32)


@pytest.mark.parametrize("kind", ["smooth", "large", "leaving", "integer"])
def test_brute_force_matches_scipy_griddata(kind):
    """The test's float64 brute force IS the reference's forward_interpolate (wrap=False): griddata(..., method='nearest') of
    the valid moved points, wherever the nearest point is unique by more than 1e-3 px; at (near) ties scipy's choice is one of
    the points within 1e-3 px of the minimum, as the brute force's is."""
    interpolate = pytest.importorskip("scipy.interpolate")
    h, w = 24, 40
    flow = flows(kind, h, w, seed=3)
    x1, y1, valid = fref.moved_points(flow, wrap=False)
    x0, y0 = np.meshgrid(np.arange(w), np.arange(h))
    pts = (x1[valid], y1[valid])
    fx = interpolate.griddata(pts, flow[0].reshape(-1)[valid], (x0, y0), method="nearest", fill_value=0)
    fy = interpolate.griddata(pts, flow[1].reshape(-1)[valid], (x0, y0), method="nearest", fill_value=0)
    ref = np.stack([fx, fy]).astype(np.float32)
    n_unique = fref.check(ref, flow, wrap=False)         # scipy's answer passes the bar the kernel is held to
    vals, idx, d_min, d_second = fref.nearest(flow, wrap=False)
    unique = np.sqrt(d_second) - np.sqrt(d_min) > 1e-3
    assert n_unique == unique.sum() and unique.mean() > (0.3 if kind == "integer" else 0.9)
    assert np.array_equal(ref.reshape(2, -1)[:, unique], vals[:, unique])


def _emu_run(emu, flow_b2hw: np.ndarray, wrap: bool) -> np.ndarray:
    B, _, h, w = flow_b2hw.shape
    f = torch.from_numpy(np.ascontiguousarray(flow_b2hw))
    out = torch.full_like(f, float("nan"))
    scratch = torch.zeros(emu.forward_interpolate_scratch_bytes(B, h, w) // 4, dtype=torch.int32)
    emu.forward_interpolate(f, out, scratch, wrap=wrap)
    return out.numpy()


@pytest.mark.parametrize("wrap", [False, True])
@pytest.mark.parametrize("kind,h,w", [("smooth", 16, 32), ("large", 16, 32), ("leaving", 20, 24), ("integer", 16, 32),
                                      ("invalid", 16, 32), ("large", 64, 128)])
def test_emulated_forward_interpolate_matches_brute_force(emu, kind, h, w, wrap):
    """The kernel's element forms (count, scan, scatter, ring search) on the host equal the float64 brute force bit for bit,
    ties included (both take the lowest source index), and pass the issue's bar."""
    flow = np.stack([flows(kind, h, w, seed=s) for s in (1, 2)])          # B = 2
    out = _emu_run(emu, flow, wrap)
    for b in range(2):
        vals, idx, _, _ = fref.nearest(flow[b], wrap)
        assert np.array_equal(out[b].reshape(2, -1), vals), (b, int((out[b].reshape(2, -1) != vals).any(0).sum()))
        fref.check(out[b], flow[b], wrap)
    if kind == "invalid":
        assert not out.any()


def test_emulated_forward_interpolate_edges(emu):
    """Zero flow: column 0 and row 0 are not valid points (strict inequalities), so they take their neighbours' values; with
    wrap the x test always holds and column 0 stays, a point moved past the right edge comes back on the left."""
    h, w = 8, 16
    flow = np.zeros((1, 2, h, w), np.float32)
    flow[0, 0] = np.arange(w, dtype=np.float32)[None, :] * 0.01
    out = _emu_run(emu, flow, wrap=False)
    assert np.array_equal(out[0, 0, :, 0], flow[0, 0, :, 1])             # column 0 dropped: nearest is column 1
    out = _emu_run(emu, flow, wrap=True)
    assert np.array_equal(out[0, 0, 1:], flow[0, 0, 1:])                 # everything but row 0 stays put
    flow = np.zeros((1, 2, h, w), np.float32)
    flow[0, 0, 3, w - 1] = 1.25                                          # (15, 3) -> (16.25, 3) = (0.25, 3) modulo 16
    flow[0, 1] = 0.0
    flow[0, 1, 0] = -5.0                                                 # row 0 leaves the frame
    out = _emu_run(emu, flow, wrap=True)
    assert out[0, 0, 3, 0] == 0.0 and out[0, 0, 3, w - 1] == 0.0         # target (0, 3) keeps its own zero-flow point
    fref.check(out[0], flow[0], True)


def test_emulated_prepare_frame_equals_prepare_images(emu):
    """pf_prepare_frame = the image1 half of pf_prepare_images (img_c), bit for bit."""
    import math
    from prior_flow_amd.engine import rotation_x
    B, H, W = 2, 16, 32
    g = torch.Generator().manual_seed(0)
    i1 = torch.rand(B, 3, H, W, generator=g) * 255
    i2 = torch.rand(B, 3, H, W, generator=g) * 255
    grid = torch.zeros(2, H, W)
    emu.sample_grid(grid, rotation_x(-math.pi / 2))
    f, c = torch.zeros(4 * B, 3, H, W), torch.zeros(2 * B, 3, H, W)
    emu.prepare_images(i1, i2, grid, f, c)
    out = torch.full((2 * B, 3, H, W), float("nan"))
    emu.prepare_frame(i1, grid, out)
    assert torch.equal(out, c)


def test_new_entry_points_refuse_bad_arguments(emu):
    """PF_ERR_* before any launch, in the emulation build (and the device build when it has been built)."""
    libs = [ctypes.CDLL(EMU_SO)]
    from prior_flow_amd import _lib
    if os.path.exists(_lib.LIB_PATH):
        libs.append(ctypes.CDLL(_lib.LIB_PATH))
    buf = (ctypes.c_float * 1024)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    q = ctypes.c_void_p(ctypes.addressof(buf) + 2048)
    for dll in libs:
        for name in NEW:
            assert hasattr(dll, name)
        fi = dll.pf_forward_interpolate
        fi.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long] + [ctypes.c_int] * 4 + [ctypes.c_void_p]
        assert fi(None, q, p, 4096, 1, 4, 4, 0, None) == -1                  # NULL flow
        assert fi(p, p, q, 4096, 1, 4, 4, 0, None) == -1                     # flow == out
        assert fi(p, q, None, 4096, 1, 4, 4, 0, None) == -1                  # no scratch
        assert fi(p, q, p, 4096, 1, 4, 4, 2, None) == -1                     # wrap not 0 / 1
        assert fi(p, q, p, 4 * (3 * 16 + 1) - 1, 1, 4, 4, 0, None) == -1     # scratch one byte short
        assert fi(p, q, p, 4096, 0, 4, 4, 0, None) == -2                     # empty batch
        pr = dll.pf_prepare_frame
        pr.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 3 + [ctypes.c_void_p]
        assert pr(None, p, q, 1, 16, 32, None) == -1
        assert pr(p, p, p, 1, 16, 32, None) == -1                            # out == image
        assert pr(p, q, ctypes.c_void_p(ctypes.addressof(buf) + 1024), 0, 16, 32, None) == -2   # empty batch
    from prior_flow_amd._lib import PfError
    with pytest.raises(PfError):
        emu.forward_interpolate(torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 4, 4), torch.zeros(64, dtype=torch.int32))
    with pytest.raises(PfError):                                             # scratch too small
        emu.forward_interpolate(torch.zeros(1, 2, 4, 4), torch.zeros(1, 2, 4, 4), torch.zeros(4, dtype=torch.int32))
    with pytest.raises(PfError):
        emu.prepare_frame(torch.zeros(1, 3, 16, 32), torch.zeros(2, 16, 32), torch.zeros(1, 3, 16, 32))


def test_python_forward_interpolate_needs_a_device_tensor():
    """evaluate.forward_interpolate has no CPU path."""
    from prior_flow_amd import evaluate
    from prior_flow_amd._lib import PfError
    with pytest.raises(PfError):
        evaluate.forward_interpolate(torch.zeros(2, 16, 32))
