"""Seeded inputs, the stored cases and hand-written parameter tables of the augmentation tests -- TEST INFRASTRUCTURE ONLY.

The inputs are regenerated from seeds (numpy's legacy RandomState stream is frozen) and stored in tests/golden/augment_360.npz
as well; the tests read the stored ones.  ``CASES`` lists the reference runs of the fixture (tests/gen_golden_augment.py): size,
seed (``np.random.seed(s); torch.manual_seed(s)`` on the reference, ``RandomState(s)`` / ``manual_seed(s)`` for
``sample_params_360``), whether the reference ran with ``asymmetric_rotaton_aug_prob = 1.0``, whether its colour step was the
identity (ColorJitter(0, 0, 0, 0); blocky input images, which compress; their flows are not stored), and the features the case was chosen for.
"""
from __future__ import annotations

import numpy as np

SIZES = ((64, 128), (72, 150))            # W = 150 is no multiple of 4
OP_FACTORS = (0.6, 0.83, 1.0, 1.21, 1.4)  # single-operation factors of bar 1
HUE_SHIFTS = (14, 128, 243)
OP_SIZE = (16, 32)                        # the single-operation images: noise and a ramp
HSV_SIZE = (32, 64)
# input seeds per size: noise images whose mean(L), alone and stacked, is at least 0.15 away from .5 (the contrast-first cases)
INPUT_SEED = {(64, 128): 1, (72, 150): 6}

# (name, (H, W), seed, asymmetric roll on the reference, identity colour, features the generator asserts)
CASES = (
    ("a", (64, 128), 11, False, False, ("asym", "contrast_first", "contrast_last", "contrast_after_hue", "two_rects", "clip_right",
                                        "clip_bottom", "no_roll")),
    ("b", (64, 128), 29, False, False, ("sym", "contrast_first", "one_rect", "roll_pos", "seam")),
    ("c", (64, 128), 1, False, False, ("sym", "no_eraser", "roll_neg")),
    ("d", (72, 150), 21, True, False, ("asym", "asym_roll", "one_rect", "seam")),
    ("e", (72, 150), 62, False, False, ("asym", "two_rects", "roll_neg", "seam")),
    ("i0", (64, 128), 15, False, True, ("two_rects", "roll_pos", "seam")),
    ("i1", (64, 128), 15, True, True, ("two_rects", "asym_roll", "seam")),
    ("i2", (72, 150), 50, False, True, ("two_rects", "roll_neg", "clip_right", "clip_bottom")),
    ("i3", (72, 150), 50, True, True, ("two_rects", "asym_roll", "seam")),
)
# every one of these appears in at least one case of the fixture (asserted by the generator and by the host test)
REQUIRED = ("sym", "asym", "contrast_first", "contrast_last", "contrast_after_hue", "no_eraser", "one_rect", "two_rects",
            "clip_right", "clip_bottom", "seam", "no_roll", "roll_pos", "roll_neg", "asym_roll")


def tag(size):
    return f"{size[0]}x{size[1]}"


def make_images(H, W, seed):
    """Two uint8 noise images [2,H,W,3]."""
    return np.random.RandomState(1000 + seed).randint(0, 256, (2, H, W, 3)).astype(np.uint8)


def make_smooth_images(H, W, seed):
    """Two images [2,H,W,3] of 4 x 4 blocks of random colours: they compress, and a roll or a rectangle misplaced by one
    pixel still shows at the block edges."""
    blocks = np.random.RandomState(3000 + seed).randint(0, 256, (2, (H + 3) // 4, (W + 3) // 4, 3)).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(np.repeat(blocks, 4, axis=1), 4, axis=2)[:, :H, :W])


def make_flow(H, W, seed):
    """fp32 [H,W,2] as decoded: multiples of 1/32 with |u| up to 1.5 W (beyond W / 2: the wrap at load acts), every eighth
    entry with a full fp32 mantissa, a few entries >= 1000 in either component, +-inf and NaN."""
    r = np.random.RandomState(2000 + seed)
    f = (r.randint(-48 * W, 48 * W, (H, W, 2)) / 32.0).astype(np.float32)
    f[..., 1] /= 4
    full = r.rand(H, W, 2) < 0.125
    f = np.where(full, (f * (1 + r.rand(H, W, 2) * 1e-3)).astype(np.float32), f).astype(np.float32)
    special = (1000.0, -1000.0, 999.9999, 1234.5, -5000.0, np.nan, np.inf, -np.inf, -0.0, W / 2, -W / 2, 1.5 * W)
    for k, v in enumerate(special):
        for c in (0, 1):
            f[r.randint(0, H), r.randint(0, W), c] = v
        f[(3 * k + 1) % H, (5 * k + 2) % W, k % 2] = v
    return f


def op_images():
    """The inputs of the single-operation checks [2, h, w, 3]: noise and a ramp."""
    h, w = OP_SIZE
    noise = np.random.RandomState(77).randint(0, 256, (h, w, 3))
    y, x = np.mgrid[0:h, 0:w]
    ramp = np.stack([(x * 255) // (w - 1), (y * 255) // (h - 1), ((x + y) * 255) // (w + h - 2)], -1)
    return np.stack([noise, ramp]).astype(np.uint8)


def hsv_image():
    """Noise [H,W,3] with grey, black, white and saturated pixels mixed in: the input of the HSV conversions."""
    H, W = HSV_SIZE
    r = np.random.RandomState(78)
    img = r.randint(0, 256, (H, W, 3)).astype(np.uint8)
    img[0, :, :] = np.arange(W)[:, None] * 4                  # greys
    img[1, :, 0], img[1, :, 1], img[1, :, 2] = 255, np.arange(W) * 4, 0
    img[2, :, 0], img[2, :, 1], img[2, :, 2] = np.arange(W) * 4, 0, 255
    img[3, :, 1] = img[3, :, 0]                               # two equal maxima
    return img


def features(row, H, W):
    """The features of one parameter row (AugmentParams.row)."""
    f = {"asym" if row["asym_colour"] else "sym"}
    for s in ([row["set_a"], row["set_b"]] if row["asym_colour"] else [row["set_a"]]):
        o = s["order"]
        if o[0] == 1:
            f.add("contrast_first")
        if o[3] == 1:
            f.add("contrast_last")
        if 3 in o and 1 in o and o.index(3) < o.index(1):
            f.add("contrast_after_hue")
    f.add(("no_eraser", "one_rect", "two_rects")[len(row["rects"])])
    r2 = row["r2"] % W
    for x0, y0, dx, dy in row["rects"]:
        if x0 + dx > W:
            f.add("clip_right")
        if y0 + dy > H:
            f.add("clip_bottom")
        w = min(dx, W - x0)
        if (x0 + r2) % W + w > W:
            f.add("seam")
    if row["asym_rot"]:
        f.add("asym_roll")
    elif row["r1"] == 0:
        f.add("no_roll")                  # rotation off, or on with r = 0: the same output
    else:
        f.add("roll_pos" if row["r1"] > 0 else "roll_neg")
    return f


def identity_colour(params, b=0):
    """Overwrite the colour sets of row b with the identity: factors 1 and no hue step (a hue step with shift 0 is PIL's
    RGB -> HSV -> RGB round trip, which is not the identity)."""
    params.set_asymmetric_colour(b, False)
    for second in (False, True):
        params.set_colour(b, (0, 1, 2, 4), 1.0, 1.0, 1.0, shift=0, second=second)
    return params


def hand_cases(H, W):
    """Geometry cases with the table filled by hand: (name, rects, r1, r2 or None)."""
    m = int(np.round(0.2 * W))
    return (("rect at x0 = W - 1", [(W - 1, 5, 60, 50)], 7, None),
            ("rect inside", [(10, 8, 50, 40)], -9, None),
            ("two overlapping rects", [(20, 10, 60, 30), (50, 25, 55, 60)], 13, None),
            ("r = -round(0.2 W)", [(W - 30, H - 20, 99, 99)], -m, None),
            ("r = 0 with rotation on", [(0, 0, 50, 50)], 0, None),
            ("asymmetric rolls", [(W - 3, 0, 50, H + 5)], m - 1, -m))


# ---- the fixture and the shared checks -------------------------------------------------------------------------------------
def golden():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "augment_360.npz"))


def case_inputs(g, case):
    """(img [2,H,W,3] uint8, flow [H,W,2] fp32) of a stored case."""
    name, size, seed, asym_roll, identity, _ = case
    return g[("smooth_" if identity else "img_") + tag(size)], g["flow_" + tag(size)]


def case_expected(g, case):
    """The reference's outputs as the loader delivers them (core/datasets.py:152-159): image1, image2 [3,H,W] fp32, flow_gt
    [2,H,W] and valid [H,W] (None, None for the identity cases, whose flows are not stored)."""
    name = case[0]
    i1, i2 = (g[f"{name}_img{k}"].transpose(2, 0, 1).astype(np.float32) for k in (1, 2))
    if f"{name}_flow" not in g.files:
        return i1, i2, None, None
    fl = np.ascontiguousarray(g[f"{name}_flow"].transpose(2, 0, 1))
    with np.errstate(invalid="ignore"):
        valid = ((np.abs(fl[0]) < 1000) & (np.abs(fl[1]) < 1000)).astype(np.float32)
    return i1, i2, fl, valid


def case_params(case, out=None, b=0):
    """The table row of a stored case from ``sample_params_360`` with the case's seed."""
    import torch
    from prior_flow_amd import augment as ag
    name, (H, W), seed, asym_roll, identity, _ = case
    p = ag.sample_params_360(1, H, W, np.random.RandomState(seed), torch.Generator().manual_seed(seed),
                             asymmetric_rotaton_aug_prob=1.0 if asym_roll else 0.0)
    if identity:
        identity_colour(p)
    if out is not None:
        out.words[b] = p.words[0]
    return p


def run(lib, img1, img2, flow, params, device="cpu"):
    """pf_augment_360 through a PfLib handle (the emulation on the host, the product's library on a device): numpy in, numpy out."""
    import torch
    B, H, W, _ = img1.shape
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
    out = [torch.full(s, float("nan"), device=device) for s in ((B, 3, H, W), (B, 3, H, W), (B, 2, H, W), (B, H, W))]
    scratch = torch.zeros(lib.augment_scratch_bytes(B) // 8, dtype=torch.int64, device=device)
    lib.augment_360(t(img1), t(img2), t(flow), t(params.words), *out, scratch)
    return [o.cpu().numpy() for o in out]


def image_diff(got, want):
    """(share of differing bytes, largest difference in levels) between images."""
    d = np.abs(np.asarray(got, np.float32) - np.asarray(want, np.float32))
    return float((d != 0).mean()), float(d.max())


# the cap of DESIGN.md section 14 on anything that contains RGB -> HSV: at most 0.5 % of bytes differ, a lone hue step by at most
# 7 levels, a whole chain by at most 28
CAP_SHARE, CAP_HUE, CAP_CHAIN = 0.005, 7, 28


def same_flow(got, want):
    """Bit for bit, NaN where the reference has NaN (a NaN's payload is not compared)."""
    return np.array_equal(got, want, equal_nan=True) and np.array_equal(np.signbit(got[~np.isnan(got)]), np.signbit(want[~np.isnan(want)]))


def one_op_params(op, factor=1.0, shift=0):
    """A one-row table whose colour step is one operation alone (the other three steps skipped)."""
    from prior_flow_amd import augment as ag
    p = ag.AugmentParams(1)
    f = [1.0, 1.0, 1.0]
    if op < 3:
        f[op] = factor
    for second in (False, True):
        p.set_colour(0, (op, 4, 4, 4), f[0], f[1], f[2], shift=shift, second=second)
    return p


def hand_params(H, W, rects, r1, r2):
    from prior_flow_amd import augment as ag
    return ag.AugmentParams(1).set_rects(0, rects).set_roll(0, r1, r2)


# Shapes at which pf_aug_blocks caps a grid at 1024 workgroups, so that its threads go round their loops a second time
# (tests/launch_paths.py: augment_grids): (B, H, W) = (1, 514, 2048), four pixels per thread in the main kernel, where rows 512 and
# 513 are the second trip of the main kernel AND of the contrast pass; (2, 258, 1018), one pixel per thread, where the last 500
# pixels are.  CAPPED_RECT holds 12 000 pixels: more than the 10 240 threads of the eraser's grid.
CAPPED = ((1, 514, 2048), (2, 258, 1018))
CAPPED_RECT = (10, 20, 120, 100)


def capped_batch(shape):
    """(img1, img2, flow, params, row0) of a CAPPED shape.  No hue step (RGB -> HSV is the one operation on which device and
    emulation may differ): the chain is exact, so every byte is compared.  The frames are noise in [41, 160), mean L = 100.0, with
    the rows from row0 = 512 on white at H = 514: the mean of L over the stacked pair is 100.60 with them and 99.61 when their sum
    is left out, int(mean + 0.5) = 101 against 100 (contrast_means).  The contrast step comes second, behind a brightness step
    of factor 1, in sample 0, third in the first set of sample 1 and first in its second set."""
    from prior_flow_amd import augment as ag
    B, H, W = shape
    r = np.random.RandomState(17 + H)
    i1, i2 = (r.randint(41, 160, (B, H, W, 3)).astype(np.uint8) for _ in range(2))
    row0 = 512 if H > 512 else H
    i1[:, row0:], i2[:, row0:] = 255, 255
    fl = np.stack([make_flow(H, W, 60 + b) for b in range(B)])
    p = ag.AugmentParams(B)
    for second in (False, True):
        p.set_colour(0, (0, 1, 2, 4), 1.0, 1.3, 0.8, shift=0, second=second)
    p.set_rects(0, [CAPPED_RECT, (W - 40, H - 30, 99, 99)]).set_roll(0, -101)
    if B > 1:
        p.set_asymmetric_colour(1).set_colour(1, (2, 0, 1, 4), 1.2, 0.7, 1.1, shift=0)
        p.set_colour(1, (1, 2, 4, 0), 0.9, 1.35, 1.25, shift=0, second=True)
        p.set_rects(1, [CAPPED_RECT]).set_roll(1, 57, -60)          # the rolled rectangle straddles the seam
    return i1, i2, fl, p.validate(H, W), row0


def contrast_means(i1, i2, row0):
    """int(mean(L) + 0.5) of the stacked pair (augment_ref.contrast_mean), and the same with the sum of the rows from row0 left
    out of the numerator only: what a contrast pass that drops its second trip would hand to the main kernel."""
    import augment_ref as ar
    n = 2 * i1.shape[0] * i1.shape[1]
    s = sum(int(ar.luma(i[:row0]).astype(np.int64).sum()) for i in (i1, i2))
    return ar.contrast_mean([i1, i2]), (2 * s + n) // (2 * n)


def small_odd_batch():
    """Three samples of 5 x 7 (H * W = 35, no multiple of 4): symmetric colour with the contrast step third, asymmetric colour with
    contrast second and last, and contrast first; a clipped rectangle each, symmetric and asymmetric rolls.  With 35 pixels
    0.5 % of the bytes is less than one byte: the cap allows no differing byte at this size."""
    from prior_flow_amd import augment as ag
    H, W, B = 5, 7, 3
    r = np.random.RandomState(55)
    i1, i2 = (r.randint(0, 256, (B, H, W, 3)).astype(np.uint8) for _ in range(2))
    fl = (r.standard_normal((B, H, W, 2)) * 9).astype(np.float32)
    fl[0, 1, 2, 0], fl[1, 4, 6, 1], fl[2, 0, 0, 0] = np.nan, 1000.0, -17.25
    p = ag.AugmentParams(B)
    p.set_colour(0, (0, 3, 1, 2), 1.3, 0.7, 1.2, shift=31).set_colour(0, (0, 3, 1, 2), 1.3, 0.7, 1.2, shift=31, second=True)
    p.set_rects(0, [(5, 3, 60, 60)]).set_roll(0, 3)
    p.set_asymmetric_colour(1).set_colour(1, (2, 1, 3, 0), 0.8, 1.35, 0.9, shift=220).set_colour(1, (3, 0, 2, 1), 1.1, 0.65, 1.4, shift=5, second=True)
    p.set_rects(1, [(0, 0, 2, 2), (6, 4, 50, 50)]).set_roll(1, 2, -1)
    p.set_colour(2, (1, 0, 2, 3), 0.9, 1.25, 1.1, shift=128).set_colour(2, (1, 0, 2, 3), 0.9, 1.25, 1.1, shift=128, second=True)
    p.set_roll(2, -1)
    return i1, i2, fl, p.validate(H, W)
