"""Shared by tests/test_flow_viz_host.py (host emulation) and tests/test_hip_flow_viz.py (device): runners of the four entry points
through the binding on numpy arrays, the input kinds of the order statistic, and the bars of DESIGN.md section 13."""
import os

import numpy as np
import torch

import flow_viz_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = [os.path.join(ROOT, "tests", "golden", n) for n in ("flow_viz.npz", "flow_viz_warp.npz")]

# Colour bytes: every value within 1 of the reference and at most 0.5 % of the values different (atan2f / asinf at a few ulp give
# ~5e-7 in the angle, x 27 into the wheel index, x 64 for the steepest wheel segment -> ~1e-3 in 255 col, so ~2e-3 of the values
# of the steepest segments can sit on the other side of a floor).
COLOUR_MAX_DIFF = 1
COLOUR_MAX_SHARE = 0.005
# Warp: seven fp32 roundings on the path of a tap x 2^-24 x 255 ~ 1.1e-4, doubled.
WARP_ATOL = 2e-4
# Great-circle length against the reference's: the bar tests/test_hip_eval.py holds the same haversine distance to.
SD_ATOL = 2e-6
# mean_err: a sum of <= 2^20 non-negative floats reduced in a tree
MEAN_ERR_RTOL = 1e-5

OS_KINDS = ("random", "tied", "equal", "zero", "inf", "nan")

# Shapes at which pf_os_blocks caps the grid at 2048 workgroups, so that some thread goes round its loop once more than at any
# smaller size (tests/launch_paths.py: os_grid, render_grids): a selection pass of 8 items per thread beyond 4 194 304 values, the
# one-pixel length and colour kernels beyond 524 288 pixels (W % 4 != 0), the four-pixel ones beyond 524 288 quads.
OS_CAPPED_N = 4200000
OS_CAPPED_KINDS = ("random", "tied")
RENDER_CAPPED = ((258, 2034), (1026, 2048))


def golden():
    """The arrays of both fixture files (the second holds the images and the reference's my_cycle_warp of them)."""
    out = {}
    for path in GOLDEN:
        with np.load(path) as z:
            out.update({k: z[k] for k in z.files})
    return out


# (H, W, C) of the warp cases that have the reference's result: the stored channels, and their first channel alone
WARP_CASES = [(H, W, C) for (H, W), n in sorted(fc.FIXTURE_WARP.items()) for C in sorted({1, n})]


def os_input(kind, B, n, seed=0):
    rng = np.random.default_rng(seed)
    x = np.abs(rng.standard_normal((B, n))).astype(np.float32) * np.float32(0.3)
    if kind == "tied":
        x = (np.floor(x * 16) / 16).astype(np.float32)           # 16 levels (and a few above)
        x = np.minimum(x, np.float32(15 / 16))
    elif kind == "equal":
        x[:] = np.float32(0.7312)
    elif kind == "zero":
        x[:] = 0
    elif kind == "inf":
        x[:, rng.integers(0, n, size=max(2, n // 50))] = np.inf
    elif kind == "nan":
        x[:, rng.integers(0, n, size=max(2, n // 20))] = np.nan
    return x


def os_ranks(n):
    return sorted({0, 1, int(0.95 * n), n - 2, n - 1})


def os_expected(x, k):
    """np.sort(x[b])[k]; when that is NaN: the largest value that is not (0 when there is none)."""
    out = np.empty(len(x), np.float32)
    for b in range(len(x)):
        s = np.sort(x[b])
        v = s[k]
        if np.isnan(v):
            good = s[~np.isnan(s)]
            v = good[-1] if len(good) else np.float32(0)
        out[b] = v
    return out


def _dev(a, device):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t if device is None else t.to(device)


def run_order_stat(lib, x, k, device=None, repeats=1):
    t = _dev(x, device)
    B, n = t.shape
    scratch = torch.full((lib.order_stat_scratch_bytes(B, n) // 4,), -1, dtype=torch.int32, device=t.device)   # dirty on purpose
    outs = []
    for _ in range(repeats):
        out = torch.full((B,), -5.0, dtype=torch.float32, device=t.device)
        lib.order_stat(t, k, out, scratch)
        outs.append(out.cpu().numpy())
    return outs if repeats > 1 else outs[0]


def run_render(lib, flow, mode="omni", percentile=0.95, layout="hwc", bgr=False, device=None, offset=0):
    """-> (image, len [B,H,W], clip [B]).  offset: element offset of the flow inside its allocation (4: still 16-byte aligned;
    1: forces the one-pixel-per-thread path on the device)."""
    B, _, H, W = flow.shape
    buf = torch.zeros(flow.size + offset, dtype=torch.float32)
    buf[offset:] = torch.from_numpy(np.ascontiguousarray(flow)).reshape(-1)
    if device is not None:
        buf = buf.to(device)
    f = buf[offset:].view(B, 2, H, W)
    scratch = torch.full(((lib.flow_render_scratch_bytes(B, H, W) + 3) // 4,), -1, dtype=torch.int32, device=f.device)
    out = torch.full((B, H, W, 3) if layout == "hwc" else (B, 3, H, W), 77, dtype=torch.uint8, device=f.device)
    lib.flow_render(f, out, scratch, mode=mode, percentile=percentile, layout=layout, bgr=bgr)
    fl = scratch.view(torch.float32)
    N = B * H * W
    return out.cpu().numpy(), fl[:N].view(B, H, W).cpu().numpy().copy(), fl[N:N + B].cpu().numpy().copy()


def run_warp(lib, x, flo, ref=None, device=None):
    """-> (warped, err or None)"""
    xt, ft = _dev(x, device), _dev(flo, device)
    out = torch.full_like(xt, float("nan"))
    if ref is None:
        lib.cycle_warp(xt, ft, out)
        return out.cpu().numpy(), None
    err = torch.full((xt.shape[0],) + tuple(xt.shape[2:]), float("nan"), dtype=torch.float32, device=xt.device)
    lib.cycle_warp(xt, ft, out, ref=_dev(ref, device), err=err)
    return out.cpu().numpy(), err.cpu().numpy()


def run_masked_mean(lib, x, mask, device=None):
    xt = _dev(x, device)
    out = torch.full((xt.shape[0],), float("nan"), dtype=torch.float32, device=xt.device)
    scratch = torch.zeros(128 * xt.shape[0], dtype=torch.float64, device=xt.device)
    lib.masked_mean(xt, None if mask is None else _dev(mask, device), out, scratch)
    return out.cpu().numpy()


def colour_figures(got, want, what):
    """Print and return (largest difference, share of differing values); assert the bars."""
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    mx, share = int(d.max()), float((d != 0).mean())
    print(f"[flow_viz] {what}: max byte difference {mx}, differing share {share:.3e}")
    assert mx <= COLOUR_MAX_DIFF, (what, mx)
    assert share <= COLOUR_MAX_SHARE, (what, share)
    return mx, share


def fixture_flow(g, H, W):
    return g[f"flow_{H}x{W}"].astype(np.float32)


def big_case(B=2, H=512, W=1024, seed=77):
    return fc.make_flow(B, H, W, seed), fc.make_image(B, 3, H, W, seed)
