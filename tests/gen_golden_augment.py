"""Emit tests/golden/augment_360.npz: the reference's FlowAugmentor_360 on seeded samples, and PIL's single operations.

Run only where the reference tree and Pillow are present:  ``python tests/gen_golden_augment.py``  (``--search`` lists, per
size, seeds and the features their samples show, for choosing tests/augment_cases.CASES; ``--hsv`` runs only the exhaustive
comparison of the restated HSV conversions with Pillow, which every full run asserts as well).  The fixture holds data only: the
inputs (tests/augment_cases.py), per case what ``FlowAugmentor_360.__call__`` returns for them after the loader's u-wrap
(core/datasets.py:138) under ``np.random.seed(s); torch.manual_seed(s)``, and PIL's output for single operations.

Inert shims on top of oracle/_refharness.py: a stub ``cv2`` (imported by the augmentor for the planar classes only) and a
stand-in for ``torchvision.transforms.ColorJitter``, which is not installed: torchvision's PIL route restated with Pillow itself
(parameters from the global torch RNG in torchvision's order: randperm(4), then brightness, contrast, saturation, hue as
``uniform_`` of one element; ImageEnhance.Brightness / Contrast / Color and the HSV hue shift, tests/augment_ref.pil_op).

Asserted for every stored case: the restatement (tests/augment_ref.py driven by ``sample_params_360`` of the same seed) stays
inside the cap of DESIGN.md section 14 (its measured share of differing bytes is stored beside the case); the flow is the
reference's bit for bit; the fractional part of PIL's mean(L) at every contrast step is at least 0.05 away from .5.
"""
from __future__ import annotations

import importlib
import os
import sys
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
sys.path[:0] = [_HERE, _ROOT, os.path.join(_ROOT, "oracle")]

import augment_cases as ac  # noqa: E402
import augment_ref as ar  # noqa: E402
from _refharness import load_reference  # noqa: E402

MEANS = []          # PIL's mean(L) at every contrast step of the current run


class ColorJitter:
    """torchvision.transforms.ColorJitter on PIL images, restated (see the module docstring)."""

    def __init__(self, brightness=0, contrast=0, saturation=0, hue=0):
        rng = lambda v: None if v == 0 else (max(0.0, 1.0 - v), 1.0 + v)  # noqa: E731
        self.ranges = [rng(brightness), rng(contrast), rng(saturation), None if hue == 0 else (-hue, hue)]

    def __call__(self, img):
        from PIL import Image, ImageStat
        order = torch.randperm(4).tolist()
        f = [None if r is None else float(torch.empty(1).uniform_(r[0], r[1])) for r in self.ranges]
        arr = np.asarray(img)
        for op in order:
            if f[op] is None:
                continue
            if op == ar.OP_CONTRAST:
                MEANS.append(ImageStat.Stat(Image.fromarray(arr).convert("L")).mean[0])
            arr = ar.pil_op(arr, op, ar.hue_shift(f[op]) if op == ar.OP_HUE else f[op])
        return Image.fromarray(arr)


def load_augmentor():
    load_reference()
    cv2 = types.ModuleType("cv2")
    cv2.setNumThreads = lambda n: None
    cv2.ocl = types.SimpleNamespace(setUseOpenCL=lambda b: None)
    sys.modules.setdefault("cv2", cv2)
    if "torchvision" not in sys.modules:
        tv, tr = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms")
        tr.ColorJitter = ColorJitter
        tv.transforms = tr
        sys.modules["torchvision"], sys.modules["torchvision.transforms"] = tv, tr
    return importlib.import_module("core.utils.augmentor")


def run_reference(mod, img, flow, seed, asym_roll, identity):
    """(img1, img2, flow) of FlowAugmentor_360 on one sample, and the contrast means of the run."""
    aug = mod.FlowAugmentor_360(do_flip=False)
    if asym_roll:
        aug.asymmetric_rotaton_aug_prob = 1.0
    if identity:
        aug.photo_aug = ColorJitter(0, 0, 0, 0)
    H, W = img.shape[1:3]
    f = flow.copy()
    f[:, :, 0] = (f[:, :, 0] + W / 2) % W - W / 2           # the loader's wrap, core/datasets.py:138
    del MEANS[:]
    np.random.seed(seed)
    torch.manual_seed(seed)
    with np.errstate(invalid="ignore"):
        o1, o2, of = aug(img[0].copy(), img[1].copy(), f)
    return np.asarray(o1), np.asarray(o2), np.asarray(of, dtype=np.float32), list(MEANS)


def restated(img, flow, seed, asym_roll, identity):
    from prior_flow_amd import augment as ag
    H, W = img.shape[1:3]
    p = ag.sample_params_360(1, H, W, np.random.RandomState(seed), torch.Generator().manual_seed(seed),
                             asymmetric_rotaton_aug_prob=1.0 if asym_roll else 0.0)
    if identity:
        ac.identity_colour(p)
    with np.errstate(invalid="ignore"):
        return p.row(0), ar.augment_sample(img[0], img[1], flow, p.row(0))


def check_case(ref, mine, means, what):
    """The cap of DESIGN.md section 14 on the restatement; returns the share of differing bytes."""
    o1, o2, of, = ref
    m1, m2, mf, _ = mine
    got = np.concatenate([m1.transpose(1, 2, 0).ravel(), m2.transpose(1, 2, 0).ravel()])
    want = np.concatenate([o1.ravel(), o2.ravel()]).astype(np.float32)
    d = np.abs(got - want)
    share = float((d != 0).mean())
    assert share <= 0.005 and d.max() <= 28, (what, share, d.max())
    assert np.array_equal(mf.transpose(1, 2, 0), of, equal_nan=True), what
    for m in means:
        assert abs((m % 1.0) - 0.5) >= 0.05, (what, "mean(L) too close to .5", m)
    return share


def inputs(size, identity):
    H, W = size
    k = ac.INPUT_SEED[size]
    img = ac.make_smooth_images(H, W, k) if identity else ac.make_images(H, W, k)
    return img, ac.make_flow(H, W, k)


def search(mod, n=120):
    for size in ac.SIZES:
        for asym_roll in (False, True):
            for seed in range(n):
                img, flow = inputs(size, False)
                try:
                    ref = run_reference(mod, img, flow, seed, asym_roll, False)
                    row, mine = restated(img, flow, seed, asym_roll, False)
                    share = check_case(ref[:3], mine, ref[3], seed)
                except AssertionError as e:
                    print(ac.tag(size), seed, asym_roll, "REJECTED", e)
                    continue
                print(ac.tag(size), "seed", seed, "asym_roll", asym_roll, "share", share, sorted(ac.features(row, *size)))


def check_hsv_exhaustive():
    """The restatement's RGB -> HSV and HSV -> RGB against Pillow's Image.convert on all 2^24 triples (what DESIGN.md section 14
    states; about 20 s).  The fixture stores a small image of each direction only."""
    from PIL import Image
    a = np.arange(1 << 24, dtype=np.uint32)
    x = np.stack([(a >> 16) & 255, (a >> 8) & 255, a & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)
    for k in range(0, 4096, 512):                           # in slabs: the restatement works in float64
        slab = x[k:k + 512]
        assert np.array_equal(ar.rgb_to_hsv(slab), np.asarray(Image.fromarray(slab).convert("HSV"))), ("RGB -> HSV", k)
        assert np.array_equal(ar.hsv_to_rgb(slab), np.asarray(Image.fromarray(slab, "HSV").convert("RGB"))), ("HSV -> RGB", k)
    import PIL
    print("RGB <-> HSV: the restatement equals Pillow", PIL.__version__, "on all 2^24 triples, both directions")


def main():
    from PIL import Image
    mod = load_augmentor()
    if "--hsv" in sys.argv:
        return check_hsv_exhaustive()
    if "--search" in sys.argv:
        return search(mod)
    out, seen = {}, set()
    for size in ac.SIZES:
        out[f"img_{ac.tag(size)}"], out[f"flow_{ac.tag(size)}"] = inputs(size, False)
        out[f"smooth_{ac.tag(size)}"] = inputs(size, True)[0]
    for name, size, seed, asym_roll, identity, feats in ac.CASES:
        img, flow = inputs(size, identity)
        o1, o2, of, means = run_reference(mod, img, flow, seed, asym_roll, identity)
        row, mine = restated(img, flow, seed, asym_roll, identity)
        share = check_case((o1, o2, of), mine, means, name)
        have = ac.features(row, *size)
        assert set(feats) <= have, (name, feats, have)
        if not identity:
            seen |= have
        out[f"{name}_img1"], out[f"{name}_img2"] = o1, o2
        if not identity:
            out[f"{name}_flow"] = of
        out[f"{name}_share"] = np.float64(share)
        print(name, ac.tag(size), "seed", seed, "share of differing bytes", share, sorted(have), "means", means)
    assert set(ac.REQUIRED) <= seen, sorted(set(ac.REQUIRED) - seen)
    # PIL's single operations
    ops = ac.op_images()
    out["op_in"] = ops
    out["op_out"] = np.stack([[[ar.pil_op(im, op, float(np.float32(f))) for f in ac.OP_FACTORS] for op in range(3)] for im in ops])
    out["hue_out"] = np.stack([[ar.pil_op(im, ar.OP_HUE, s) for s in ac.HUE_SHIFTS] for im in ops])
    rgb = ac.hsv_image()
    out["hsv_in"] = rgb
    out["hsv_out"] = np.asarray(Image.fromarray(rgb).convert("HSV"))
    out["hsv_back_in"] = np.random.RandomState(79).randint(0, 256, rgb.shape).astype(np.uint8)      # any (h, s, v)
    out["hsv_back_out"] = np.asarray(Image.fromarray(out["hsv_back_in"], "HSV").convert("RGB"))
    check_hsv_exhaustive()
    path = os.path.join(_HERE, "golden", "augment_360.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)                # no committed file above 1 MiB


if __name__ == "__main__":
    main()
