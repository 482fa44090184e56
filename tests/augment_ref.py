"""numpy restatement of the 360-degree training augmentation -- TEST INFRASTRUCTURE ONLY.

What the reference's loader delivers for the 360-degree sets (core/datasets.py:137-159 with FlowAugmentor_360,
core/utils/augmentor.py:210-316), operation by operation, driven by the same parameter table the device takes
(prior_flow_amd.augment.AugmentParams).  The colour operations restate torchvision's ColorJitter on its PIL backend:
uint8 in and out after every operation, Image.blend in fp32 with truncation, PIL's 8-bit L and HSV.

``pil_chain`` is the same chain through PIL itself (ImageEnhance + the HSV hue shift): the host route that the device
path replaces, and the source of the stored single-operation outputs.
"""
from __future__ import annotations

import numpy as np

OP_BRIGHTNESS, OP_CONTRAST, OP_SATURATION, OP_HUE = 0, 1, 2, 3


def luma(img):
    """PIL's RGB -> L: (19595 R + 38470 G + 7471 B + 0x8000) >> 16."""
    i = img.astype(np.int64)
    return ((19595 * i[..., 0] + 38470 * i[..., 1] + 7471 * i[..., 2] + 0x8000) >> 16).astype(np.uint8)


def blend(deg, img, f):
    """Image.blend(degenerate, img, f): deg + f (img - deg) in fp32, clamped to [0, 255], truncated."""
    f = np.float32(f)
    d = np.asarray(deg).astype(np.float32)
    t = d + f * (img.astype(np.float32) - d)
    return np.clip(t, 0, 255).astype(np.uint8)          # 0 <= t: truncation is the floor


def brightness(img, f):
    return blend(np.zeros_like(img), img, f)


def contrast_mean(imgs):
    """int(mean(L) + 0.5) over all the images given (one PIL image: the vertical stack in the symmetric mode)."""
    s = sum(int(luma(i).astype(np.int64).sum()) for i in imgs)
    n = sum(i.shape[0] * i.shape[1] for i in imgs)
    return (2 * s + n) // (2 * n)


def contrast(img, f, mean=None):
    m = contrast_mean([img]) if mean is None else mean
    return blend(np.full_like(img, m), img, f)


def saturation(img, f):
    return blend(np.repeat(luma(img)[..., None], 3, axis=2), img, f)


def rgb_to_hsv(img):
    """PIL's 8-bit RGB -> HSV: h = fmod((h6 / 6 + 1), 1) from fp32 ratios, widened to double for the last steps; bytes by
    truncation of 255 h and 255 s."""
    r, g, b = (img[..., c].astype(np.int32) for c in range(3))
    maxc, minc = np.maximum(np.maximum(r, g), b), np.minimum(np.minimum(r, g), b)
    cr = np.maximum(maxc - minc, 1).astype(np.float32)
    s = cr / np.maximum(maxc, 1).astype(np.float32)
    rc, gc, bc = ((maxc - c).astype(np.float32) / cr for c in (r, g, b))
    h = np.where(r == maxc, (bc - gc).astype(np.float64),
                 np.where(g == maxc, 2.0 + rc.astype(np.float64) - bc.astype(np.float64),
                          4.0 + gc.astype(np.float64) - rc.astype(np.float64))).astype(np.float32)
    h = np.fmod(h.astype(np.float64) / 6.0 + 1.0, 1.0).astype(np.float32)
    uh = np.clip((h.astype(np.float64) * 255.0).astype(np.int32), 0, 255)
    us = np.clip((s.astype(np.float64) * 255.0).astype(np.int32), 0, 255)
    grey = maxc == minc
    return np.stack([np.where(grey, 0, uh), np.where(grey, 0, us), maxc], axis=-1).astype(np.uint8)


def hsv_to_rgb(hsv):
    """PIL's 8-bit HSV -> RGB: sector i = floor(6 h / 255), p, q, t rounded half away from zero."""
    h, s, v = (hsv[..., c].astype(np.float32) for c in range(3))
    h6 = h.astype(np.float64) * 6.0 / 255.0
    i = np.floor(h6).astype(np.float32).astype(np.int32)
    f = (h6 - i.astype(np.float32).astype(np.float64)).astype(np.float32)
    fs = (s.astype(np.float64) / 255.0).astype(np.float32)
    vd, fsd, fd = v.astype(np.float64), fs.astype(np.float64), f.astype(np.float64)
    rnd = lambda x: np.clip(np.floor(x + 0.5), 0, 255).astype(np.uint8)  # noqa: E731  (arguments are >= 0)
    p, q, t = rnd(vd * (1.0 - fsd)), rnd(vd * (1.0 - fsd * fd)), rnd(vd * (1.0 - fsd * (1.0 - fd)))
    vv = hsv[..., 2]
    sel = i % 6
    table = [(vv, t, p), (q, vv, p), (p, vv, t), (p, q, vv), (t, p, vv), (vv, p, q)]
    out = np.zeros(hsv.shape, np.uint8)
    for k, chans in enumerate(table):
        for c in range(3):
            out[..., c] = np.where(sel == k, chans[c], out[..., c])
    grey = hsv[..., 1] == 0
    for c in range(3):
        out[..., c] = np.where(grey, vv, out[..., c])
    return out


def hue_shift(f):
    """The byte torchvision adds to the hue plane: trunc(255 f) mod 256 (f: the fp32 draw, the product in double)."""
    return int(np.trunc(float(np.float32(f)) * 255)) & 255


def hue(img, shift):
    hsv = rgb_to_hsv(img)
    hsv[..., 0] = ((hsv[..., 0].astype(np.int32) + int(shift)) & 255).astype(np.uint8)
    return hsv_to_rgb(hsv)


def jitter(imgs, order, fb, fc, fs, shift):
    """One ColorJitter draw applied to one PIL image that is the vertical stack of ``imgs``."""
    imgs = [i.copy() for i in imgs]
    for op in order:
        if op == OP_BRIGHTNESS:
            imgs = [brightness(i, fb) for i in imgs]
        elif op == OP_CONTRAST:
            m = contrast_mean(imgs)
            imgs = [contrast(i, fc, m) for i in imgs]
        elif op == OP_SATURATION:
            imgs = [saturation(i, fs) for i in imgs]
        elif op == OP_HUE:                                   # any other value: the step is skipped
            imgs = [hue(i, shift) for i in imgs]
    return imgs


def u_clip(u, W):
    return (u + W / 2) % W - W / 2


def augment_sample(img1, img2, flow, row):
    """One sample through the whole chain.  img1, img2: uint8 [H,W,3]; flow: fp32 [H,W,2] as decoded (before the u-wrap);
    row: one row of an AugmentParams table (AugmentParams.row(b) gives the dictionary used here).
    Returns image1 [3,H,W], image2, flow_gt [2,H,W], valid [H,W], all fp32."""
    H, W = img1.shape[:2]
    flow = flow.astype(np.float32).copy()
    flow[:, :, 0] = u_clip(flow[:, :, 0], W)
    a, b = row["set_a"], row["set_b"]
    if row["asym_colour"]:
        (img1,), (img2,) = jitter([img1], **a), jitter([img2], **b)
    else:
        img1, img2 = jitter([img1, img2], **a)
    if row["rects"]:
        mean = (img2.reshape(-1, 3).astype(np.int64).sum(axis=0) // (H * W)).astype(np.uint8)
        img2 = img2.copy()
        for x0, y0, dx, dy in row["rects"]:
            img2[y0:y0 + dy, x0:x0 + dx, :] = mean
    r1, r2 = row["r1"], row["r2"]
    img1, flow, img2 = np.roll(img1, r1, axis=1), np.roll(flow, r1, axis=1), np.roll(img2, r2, axis=1)
    if row["asym_rot"]:
        flow = flow.copy()
        flow[:, :, 0] = u_clip(flow[:, :, 0] + np.float32(r2) - np.float32(r1), W)
    valid = (np.abs(flow[..., 0]) < 1000) & (np.abs(flow[..., 1]) < 1000)
    return (img1.transpose(2, 0, 1).astype(np.float32), img2.transpose(2, 0, 1).astype(np.float32),
            np.ascontiguousarray(flow.transpose(2, 0, 1)), valid.astype(np.float32))


# ---- the same colour chain through PIL (the host route; needs Pillow) -------------------------------------------------------
def pil_op(img, op, value):
    """One ColorJitter operation on torchvision's PIL backend: ImageEnhance for 0..2 (value: the factor), the HSV hue shift
    for 3 (value: the byte added to the hue plane)."""
    from PIL import Image, ImageEnhance
    im = Image.fromarray(img)
    if op == OP_HUE:
        h, s, v = im.convert("HSV").split()
        nh = ((np.asarray(h).astype(np.int32) + int(value)) & 255).astype(np.uint8)
        return np.asarray(Image.merge("HSV", (Image.fromarray(nh, "L"), s, v)).convert("RGB"))
    enh = (ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Color)[op]
    return np.asarray(enh(im).enhance(float(value)))


def pil_chain(img, order, fb, fc, fs, shift):
    for op in order:
        img = pil_op(img, op, (fb, fc, fs, shift)[op])
    return img
