"""Deterministic inputs of the flow rendering tests (tests/gen_golden_flow_viz.py stores them in the fixture; the tests rebuild
the larger ones that have no fixture)."""
import numpy as np

SIZES = ((64, 128), (128, 256), (136, 216))
FIXTURE_BATCH = {(64, 128): 2, (128, 256): 1, (136, 216): 1}      # images per size in tests/golden/flow_viz.npz
FIXTURE_WARP = {(64, 128): 3, (128, 256): 1, (136, 216): 3}      # channels of the image whose my_cycle_warp result is stored (image 0)


def make_flow(B, H, W, seed):
    """[B,2,H,W] fp32: a smooth field + noise, a block that moves 60 px across the seam, a zero-flow region; every image of the
    batch has a different field.  The values are rounded to fp16 (the fixture stores them as such, exactly)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    out = np.zeros((B, 2, H, W), np.float32)
    for b in range(B):
        ph = 0.7 * b
        u = 6.0 * np.sin(2 * np.pi * xx / W + ph) * np.cos(np.pi * yy / H) + (3.0 + 2.0 * b) * (yy / H - 0.5)
        v = 4.0 * np.cos(2 * np.pi * xx / W * (1 + b) - ph) * np.sin(np.pi * yy / H)
        u = u + 0.25 * rng.standard_normal((H, W))
        v = v + 0.25 * rng.standard_normal((H, W))
        y0, x0 = H // 4, W - W // 16                       # a block next to the seam, moving right across it
        u[y0:y0 + H // 8, x0:] = 60.0
        v[y0:y0 + H // 8, x0:] = -1.5
        u[H // 2:H // 2 + H // 6, W // 8:W // 8 + W // 5] = 0.0      # a region at rest
        v[H // 2:H // 2 + H // 6, W // 8:W // 8 + W // 5] = 0.0
        out[b, 0], out[b, 1] = u, v
    return out.astype(np.float16).astype(np.float32)


def make_image(B, C, H, W, seed):
    """[B,C,H,W] fp32 with integer values 0..255."""
    rng = np.random.default_rng(seed + 1000)
    return rng.integers(0, 256, size=(B, C, H, W)).astype(np.float32)
