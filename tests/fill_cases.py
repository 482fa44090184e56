"""Cases and runners shared by tests/test_fill_host.py (the host emulation) and tests/test_hip_fill.py (the device): the emulation's
handle, the hole families and shapes of the sweep, one fill through the typed wrappers on numpy inputs (fused or level by level),
and the named property checks, each a function of a `fill(src, hole, weight) -> (out, empty)` on numpy arrays, so that the same
check runs on the emulation, on the device and on a planted fault of the restatement (tests/fill_ref.py)."""
import ctypes
import functools

import numpy as np
import torch

import fill_ref as fr

TILE_H, TILE_W = 32, 64                       # PF_FILL_TH, PF_FILL_TW
FAMILIES = ("none", "all", "one", "bern50", "bern95", "blocks", "seam", "cap", "soft", "poison_valid", "poison_holes",
            "poison_weight")
# (B, C, H, W): the smallest shapes at which each thing can go wrong -- one cell, one pull in x or y only, odd sizes, several tiles
# with ragged edges, a map of many tiles in one row, the fused tile's size and +-1 around it
SHAPES = ((1, 1, 1, 1), (2, 2, 1, 2), (1, 3, 2, 1), (3, 4, 3, 5), (1, 1, 6, 10), (2, 3, 17, 37), (1, 2, 33, 70), (3, 1, 24, 48),
          (2, 4, 64, 128), (1, 3, 40, 1100), (1, 2, TILE_H, TILE_W), (1, 4, TILE_H - 1, TILE_W - 1), (2, 1, TILE_H + 1, TILE_W + 1))
# the levels above the fifth of this one do not fit the apex kernel's LDS at C = 4: two more launches (pf_fill_plan: S = 6)
BIG = (1, 4, 300, 2300)
POISON = (np.nan, np.inf, -np.inf, 1e30, -1e30)


@functools.lru_cache(maxsize=None)
def emu():
    """PfLib handle of tests/emu/libpf_emu_fill.so (built on demand): the fill entry points, and those of the splat and of the
    depth propagation (with everything an Odometry needs) for the objects that fill their own holes."""
    import __graft_entry__ as ge
    from prior_flow_amd import _lib
    so = ge.build_emu_fill()
    keep = ("pf_fill_levels", "pf_fill_bytes", "pf_fill_pushpull", "pf_fill_stage", "pf_fill_prepare", "pf_fill_pull_level", "pf_fill_push_level",
            "pf_splat_scratch_bytes", "pf_splat_accumulate", "pf_splat_resolve", "pf_reproj_project", "pf_zsplat_bytes",
            "pf_zsplat_front", "pf_zsplat_accumulate", "pf_zsplat_resolve", "pf_depth_update")
    lib = _lib.PfLib(so, require_cuda=False, optional=tuple(n for n in _lib.EXPORTS if n not in keep))
    lib._dll.pf_emu_fill_plan.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    lib._dll.pf_emu_fill_plan.restype = None
    return lib


def plan(C, H, W):
    """(L, P, S) of a shape: the pulls, the levels of the tile kernels, the level the apex kernel streams."""
    out = (ctypes.c_int * 3)()
    emu()._dll.pf_emu_fill_plan(C, H, W, out)
    return tuple(out)


def inputs(kind, B, C, H, W, seed=0):
    """(src fp32 [B,C,H,W], hole uint8 [B,H,W], weight fp32 [B,H,W] or None) of one family."""
    rng = np.random.default_rng([seed, FAMILIES.index(kind), B, C, H, W])
    y, x = np.mgrid[0:H, 0:W]
    base = 100 + 50 * np.cos(2 * np.pi * x / W) * np.sin(np.pi * (y + 0.5) / H)
    src = np.stack([np.stack([base * (1 + 0.1 * c) + 3 * b + rng.normal(0, 2, (H, W)) for c in range(C)]) for b in range(B)])
    src = src.astype(np.float32)
    hole = np.zeros((B, H, W), np.uint8)
    weight = None
    if kind == "all":
        hole[:] = 1
    elif kind == "one":
        hole[:] = 1
        for b in range(B):
            hole[b, rng.integers(H), rng.integers(W)] = 0
    elif kind in ("bern50", "poison_valid", "poison_holes", "poison_weight", "soft"):
        hole = (rng.random((B, H, W)) < 0.5).astype(np.uint8) * np.uint8(1 + 254 * (seed % 2))
    elif kind == "bern95":
        hole = (rng.random((B, H, W)) < 0.95).astype(np.uint8)
    elif kind == "blocks":
        for b in range(B):
            for _ in range(4):
                h, w = rng.integers(1, max(2, H // 2)), rng.integers(1, max(2, W // 2))
                y0, x0 = rng.integers(H), rng.integers(W)
                hole[b, y0:y0 + h, np.arange(x0, x0 + w) % W] = 1       # a block may cross the seam
    elif kind == "seam":
        k = max(1, W // 8)
        hole[:, H // 4:max(H // 4 + 1, 3 * H // 4), :k] = 1
        hole[:, H // 4:max(H // 4 + 1, 3 * H // 4), W - k:] = 1
    elif kind == "cap":
        hole[:, :max(1, H // 4)] = 1
        hole[:, H - max(1, H // 8):] = 1
    if kind == "soft":
        weight = rng.random((B, H, W)).astype(np.float32)
        weight[rng.random((B, H, W)) < 0.1] = 0
        weight[rng.random((B, H, W)) < 0.1] = 3.0
    if kind == "poison_weight":
        weight = (0.25 + rng.random((B, H, W))).astype(np.float32)
        bad = rng.random((B, H, W)) < 0.3
        weight[bad] = rng.choice(np.float32(POISON + (0.0, -1.0)), size=int(bad.sum()))
    if kind == "poison_valid":
        bad = (rng.random((B, C, H, W)) < 0.1) & (hole[:, None] == 0)
        src[bad] = rng.choice(np.float32(POISON), size=int(bad.sum()))
    if kind == "poison_holes":
        bad = np.broadcast_to(hole[:, None] != 0, src.shape)
        src[bad] = rng.choice(np.float32(POISON), size=int(bad.sum()))
    return src, hole, weight


def sweep():
    """(kind, (B, C, H, W)) of the sweep: every family at every shape."""
    return [(k, s) for k in FAMILIES for s in SHAPES]


def _t(a, device, offset=0):
    """The array on `device`; offset: that many elements into a larger buffer (a map that is not 16-byte aligned)."""
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not offset:
        return t.to(device)
    buf = torch.zeros(t.numel() + offset, dtype=t.dtype, device=device)
    v = buf[offset:].view(t.shape)
    v.copy_(t)
    return v


def poison_scratch(f, seed=1):
    """NaN and +-1e30 all over the filler's scratch; 0xFF in empty."""
    g = torch.Generator().manual_seed(seed)
    vals = torch.tensor([float("nan"), 1e30, -1e30], dtype=torch.float32)
    f.scratch.copy_(vals[torch.randint(0, 3, (f.scratch.numel(),), generator=g)].to(f.scratch.device))
    f.empty.fill_(255)


def run(lib, src, hole, weight=None, device="cpu", form="fused", offset=0, in_place=False, filler=None):
    """One fill through prior_flow_amd.inpaint.HoleFiller on `lib`: (out [B,C,H,W], empty [B], the filler).  out is pre-filled with
    NaN, empty with 0xFF, the scratch poisoned.  form: "fused" (pf_fill_pushpull) or "levels" (the level entry points)."""
    from prior_flow_amd.inpaint import HoleFiller
    B, C, H, W = src.shape
    f = filler or HoleFiller(B, C, H, W, device, lib=lib)
    poison_scratch(f)
    s, h, w = _t(src, device, offset), _t(hole, device, offset), _t(weight, device, offset)
    out = s if in_place else _t(np.full(src.shape, np.nan, np.float32), device, offset)
    got, empty = (f.fill if form == "fused" else f.fill_levels)(s, h, w, out=out)
    assert got is out
    return out.cpu().numpy().copy(), empty.cpu().numpy().copy(), f


def filler_fn(lib, device="cpu", form="fused"):
    """fill(src [C,H,W] or [B,C,H,W], hole, weight) -> (out, empty) on numpy arrays, for the property checks."""
    def fill(src, hole, weight=None):
        one = src.ndim == 3
        if one:
            src, hole, weight = src[None], hole[None], None if weight is None else weight[None]
        out, empty, _ = run(lib, src, hole, weight, device, form)
        return (out[0], int(empty[0])) if one else (out, empty)
    return fill


def ref_fn(fault=None, dtype=np.float32):
    """The same signature on the restatement, with a planted fault when one is named."""
    def fill(src, hole, weight=None):
        if src.ndim == 3:
            r = fr.fill(src, hole, weight, dtype, fault)
            return r["out"], r["empty"]
        rs = [fr.fill(src[b], hole[b], None if weight is None else weight[b], dtype, fault) for b in range(src.shape[0])]
        return np.stack([r["out"] for r in rs]), np.array([r["empty"] for r in rs], np.uint8)
    return fill


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ---- the named checks ---------------------------------------------------------------------------------------------------------------
def check_no_holes_is_identity(fill):
    src, hole, _ = inputs("none", 2, 3, 17, 37)
    out, empty = fill(src, hole)
    assert same(out, src) and not np.any(empty)


def check_valid_pixels_keep_their_bits(fill):
    for kind in ("bern50", "blocks", "seam"):
        src, hole, _ = inputs(kind, 2, 2, 33, 70)
        src[0, 0, 0, 0] = np.float32(-0.0)
        out, _ = fill(src, hole)
        keep = np.broadcast_to(hole[:, None] == 0, src.shape)
        assert np.array_equal(bits(out)[keep], bits(src)[keep]), kind


def check_one_valid_pixel_fills_the_image(fill):
    """One valid pixel: every pixel equals it exactly, at 1x1 ... 32x64."""
    for H, W in ((1, 1), (1, 2), (2, 1), (1, 3), (2, 2), (3, 5), (4, 8), (7, 9), (16, 32), (32, 64)):
        for py, px in ((0, 0), (H - 1, W - 1), (H // 2, W // 3)):
            src = np.full((2, H, W), np.nan, np.float32)
            hole = np.ones((H, W), np.uint8)
            src[:, py, px] = (37.25, -1e-3)
            hole[py, px] = 0
            out, empty = fill(src, hole)
            assert not empty and np.all(out[0] == np.float32(37.25)) and np.all(out[1] == np.float32(-1e-3)), (H, W, py, px)


def check_all_holes_give_zeros_and_empty(fill):
    for B, C, H, W in ((1, 1, 1, 1), (2, 3, 5, 7), (1, 4, 33, 65)):
        src, hole, _ = inputs("all", B, C, H, W)
        out, empty = fill(src, hole)
        assert not bits(out).any() and np.all(np.asarray(empty) == 1), (B, C, H, W)
    src, hole, _ = inputs("bern50", 2, 2, 9, 20)
    hole[1] = 7
    out, empty = fill(src, hole)
    assert list(np.asarray(empty)) == [0, 1] and not bits(out[1]).any() and bits(out[0]).any()


def check_poison_under_holes_changes_nothing(fill):
    src, hole, _ = inputs("poison_holes", 2, 3, 24, 48)
    clean = np.where(np.broadcast_to(hole[:, None] != 0, src.shape), np.float32(0), src)
    a, ea = fill(src, hole)
    b, eb = fill(clean, hole)
    assert same(a, b) and np.array_equal(ea, eb) and np.isfinite(a).all()


def check_outputs_stay_in_range(fill, widen):
    """Every output lies within [min, max] of its image's valid values, widened by `widen(L, vmax, soft)` (0 in float64)."""
    for kind in ("bern50", "bern95", "blocks", "soft", "cap"):
        src, hole, weight = inputs(kind, 2, 2, 33, 70)
        out, _ = fill(src, hole, weight)
        for b in range(src.shape[0]):
            w0 = fr.w0_of(src[b], hole[b], None if weight is None else weight[b])
            for c in range(src.shape[1]):
                v = src[b, c][w0 > 0].astype(np.float64)
                tol = widen(fr.levels(33, 70), float(np.abs(v).max()), weight is not None)
                assert v.min() - tol <= out[b, c].min() and out[b, c].max() <= v.max() + tol, (kind, b, c)


def check_cyclic_equivariance(fill):
    """32x64, Bernoulli 0.8 holes: rolling src and hole by 16 columns (one cell of level 4) rolls out bit for bit -- exact when every
    level-4 weight is 1, which is asserted on the restatement's own pyramid first."""
    rng = np.random.default_rng(5)
    src = rng.normal(100, 30, (3, 32, 64)).astype(np.float32)
    hole = (rng.random((32, 64)) < 0.8).astype(np.uint8)
    assert np.all(fr.fill(src, hole)["pulled"][4][1] == 1)
    a, _ = fill(src, hole)
    b, _ = fill(np.roll(src, 16, axis=2), np.roll(hole, 16, axis=1))
    assert same(np.roll(a, 16, axis=2), b)


def check_pole_cap_fills_from_its_own_hemisphere(fill):
    """Rows 0..3 missing, rows 4..15 all 0, rows 16..31 all 100: the cap is exactly 0 (rows are clamped, not wrapped)."""
    src = np.zeros((1, 32, 64), np.float32)
    src[:, 16:] = 100
    hole = np.zeros((32, 64), np.uint8)
    hole[:4] = 1
    out, _ = fill(src, hole)
    assert not bits(out[:, :4]).any()


def check_known_answer_4x4(fill):
    """Block A (top left) four pixels of 0, block B (top right) one pixel of 8, the bottom blocks missing: the apex is the mean of
    the two SATURATED blocks, (0 + 8) / (1 + 1) = 4, and the bottom row, whose taps see the apex alone, is exactly 4."""
    src = np.zeros((1, 4, 4), np.float32)
    hole = np.ones((4, 4), np.uint8)
    hole[:2, :2] = 0
    hole[0, 3] = 0
    src[0, 0, 3] = 8
    out, _ = fill(src, hole)
    assert np.all(out[0, 3] == np.float32(4)), out[0]


def check_known_answer_1x3(fill):
    """[10, hole, 20]: the odd last column stands alone in the pull (level 1 is [10, 20]) and the hole at x = 1 (odd: taps 0 and 1,
    t = 0.25) is 10 + 0.25 * (20 - 10) = 12.5."""
    src = np.array([[[10, 0, 20]]], np.float32)
    hole = np.array([[0, 1, 0]], np.uint8)
    out, _ = fill(src, hole)
    assert float(out[0, 0, 1]) == 12.5, out


def quality_scene(H=32, W=64):
    """The scene of the quality check, scaled from 32x64: (image [1,H,W] float64, hole, band mask)."""
    y, x = np.mgrid[0:H, 0:W]
    k = H // 32
    img = 100 + 50 * np.cos(2 * np.pi * x / W) * np.sin(np.pi * (y + 0.5) / H) + 20 * np.sin(4 * np.pi * x / W)
    band = (y >= 10 * k) & (y < 20 * k) & ((x >= W - 4 * k) | (x < 4 * k))
    disc = (y - 8 * k) ** 2 + (x - 30 * k) ** 2 <= (5 * k) ** 2
    return img[None], (band | disc).astype(np.uint8), band


def quality_figures(fill, H=32, W=64):
    """rms error inside the holes, of the fill, of filling with the valid mean, and of the fill inside the seam band."""
    img, hole, band = quality_scene(H, W)
    out, _ = fill(img.astype(np.float32), hole)
    m = hole != 0
    rms = lambda d: float(np.sqrt(np.mean(np.square(d))))               # noqa: E731
    return rms(out[0].astype(np.float64)[m] - img[0][m]), rms(img[0][~m].mean() - img[0][m]), rms(out[0].astype(np.float64)[band] - img[0][band])


def check_quality(fill):
    got, mean_fill, _ = quality_figures(fill)
    assert got < 0.25 * mean_fill, (got, mean_fill)


# planted fault -> the check that catches it
CAUGHT_BY = {
    "push_clamps_columns": check_cyclic_equivariance,
    "push_wraps_rows": check_pole_cap_fills_from_its_own_hemisphere,
    "weight_not_saturated": check_known_answer_4x4,
    "multiply_not_select": check_poison_under_holes_changes_nothing,
    "one_level_too_few": check_one_valid_pixel_fills_the_image,
    "odd_column_pairs_with_column_0": check_known_answer_1x3,
    "taps_swapped": check_known_answer_1x3,
    "valid_overwritten": check_valid_pixels_keep_their_bits,
    "divide_by_saturated": check_known_answer_4x4,
    "apex_uninitialised": check_all_holes_give_zeros_and_empty,
}
EXACT_CHECKS = (check_no_holes_is_identity, check_valid_pixels_keep_their_bits, check_one_valid_pixel_fills_the_image,
                check_all_holes_give_zeros_and_empty, check_poison_under_holes_changes_nothing, check_cyclic_equivariance,
                check_pole_cap_fills_from_its_own_hemisphere, check_known_answer_4x4, check_known_answer_1x3, check_quality)
