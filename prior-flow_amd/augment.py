"""Training augmentation for the 360-degree sets on the device.

What the reference's loader delivers per sample -- ``FlowDataset_360.__getitem__`` with ``FlowAugmentor_360(do_flip=False)``
(core/datasets.py:137-159, core/utils/augmentor.py:210-316): the u-wrap of the ground truth, ColorJitter on torchvision's
PIL backend (symmetric on the stack of both images, or one draw per image), the eraser, the yaw roll, ``valid`` and the
planar fp32 layout -- from the decoder's uint8 HWC batch, as four launches of ``pf_augment_360``.

  * ``sample_params_360`` draws the random decisions on the host, in the reference's call order, into an ``AugmentParams``
    table (a fixed layout of 32 words per sample that a test can also fill by hand);
  * ``DeviceAugmentor360`` owns the scratch, the device copy of the table and the outputs, and launches on the current stream;
  * ``augmented_batches`` feeds a training loop: copies and augments on a side stream, ``depth`` output sets ahead.

Not built (the reference's ``__call__`` has them commented out, or they belong to other sets): ``flip_transform``,
``resize_transform``, the planar ``FlowAugmentor``, ``SparseFlowAugmentor_360`` and ``FlowAugmentor_360_ortho``; asking
for them raises ``PfError``.
"""
from __future__ import annotations

from typing import Iterable, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import PfError

ROW = _lib.AUG_ROW_WORDS
# word offsets of a row (csrc/pf_augment.h)
_MODE, _NRECT, _R1, _R2, _RECT, _SET_A, _SET_B = 0, 1, 2, 3, 4, 12, 20
ASYM_COLOUR, ASYM_ROLL = 1, 2
OP_BRIGHTNESS, OP_CONTRAST, OP_SATURATION, OP_HUE, OP_NONE = 0, 1, 2, 3, 4
# ColorJitter(brightness=0.4, contrast=0.4, saturation=0.4, hue=0.5 / 3.14), augmentor.py:220
FACTOR_RANGE = (0.6, 1.4)
HUE_RANGE = (-0.5 / 3.14, 0.5 / 3.14)
ERASER_BOUNDS = (50, 100)


def hue_shift(h: float) -> int:
    """The byte torchvision's PIL backend adds to the hue plane for a hue factor h: trunc(255 h) mod 256."""
    return int(np.trunc(float(h) * 255)) & 255


class AugmentParams:
    """The per-sample parameter table of ``pf_augment_360``: ``table`` is an int32 host tensor [B, 32] (pinned on request, so
    that it uploads without a synchronise), ``words`` its numpy view.  A fresh table is the identity: no colour change (factors
    1 and no hue step: a hue step with shift 0 is PIL's RGB -> HSV -> RGB round trip, which changes bytes), no rectangle, no roll.

    Row layout (words): 0 mode bits (1 asymmetric colour, 2 asymmetric roll); 1 number of rectangles; 2, 3 r1, r2; 4..11 two
    rectangles {x0, y0, dx, dy} (before the roll); 12..19 colour set A {order[4], brightness, contrast, saturation as fp32
    bits, hue shift}; 20..27 set B (image 2 of an asymmetric sample); 28..31 unused.
    """

    def __init__(self, B: int, pin: bool = False):
        if B < 1:
            raise PfError(f"AugmentParams: B = {B}")
        self.B = B
        self.table = torch.zeros(B, ROW, dtype=torch.int32, pin_memory=bool(pin))
        self.words = self.table.numpy()
        self.reset()

    def reset(self):
        self.words[:] = 0
        for b in range(self.B):
            for second in (False, True):
                self.set_colour(b, (OP_BRIGHTNESS, OP_CONTRAST, OP_SATURATION, OP_NONE), 1.0, 1.0, 1.0, shift=0, second=second)
        return self

    def set_colour(self, b: int, order: Sequence[int], brightness: float, contrast: float, saturation: float,
                   hue: Optional[float] = None, shift: Optional[int] = None, second: bool = False):
        """One ColorJitter draw: the order of the four operations (OP_*; OP_NONE skips a step) and their factors; the hue as
        torchvision's factor ``hue`` or directly as the byte ``shift`` added to the hue plane."""
        if len(order) != 4 or (hue is None) == (shift is None):
            raise PfError("set_colour: four operations, and either hue or shift")
        w = self.words[b, (_SET_B if second else _SET_A):][:8]
        w[:4] = [int(o) for o in order]
        w[4:7] = np.array([brightness, contrast, saturation], np.float32).view(np.int32)
        w[7] = hue_shift(hue) if shift is None else int(shift) & 255
        return self

    def set_asymmetric_colour(self, b: int, on: bool = True):
        self.words[b, _MODE] = (int(self.words[b, _MODE]) & ~ASYM_COLOUR) | (ASYM_COLOUR if on else 0)
        return self

    def set_rects(self, b: int, rects: Sequence[Sequence[int]]):
        """Up to two eraser rectangles (x0, y0, dx, dy), in the image before the roll; clipped at the border by the kernel."""
        if len(rects) > 2:
            raise PfError("set_rects: at most two rectangles")
        self.words[b, _NRECT] = len(rects)
        self.words[b, _RECT:_RECT + 8] = 0
        for k, r in enumerate(rects):
            self.words[b, _RECT + 4 * k:_RECT + 4 * k + 4] = [int(v) for v in r]
        return self

    def set_roll(self, b: int, r1: int, r2: Optional[int] = None):
        """Roll by whole pixels: the symmetric form (r2 None: both images and the flow by r1, flow values unchanged) or the
        asymmetric one (image 1 and the flow by r1, image 2 by r2, u = u_clip((u + r2) - r1))."""
        self.words[b, _R1] = int(r1)
        self.words[b, _R2] = int(r1 if r2 is None else r2)
        self.words[b, _MODE] = (int(self.words[b, _MODE]) & ~ASYM_ROLL) | (0 if r2 is None else ASYM_ROLL)
        return self

    def row(self, b: int) -> dict:
        """Row b as a dictionary (what tests/augment_ref.py takes)."""
        w = self.words[b]

        def cset(o):
            f = w[o + 4:o + 7].view(np.float32)
            return dict(order=[int(v) for v in w[o:o + 4]], fb=float(f[0]), fc=float(f[1]), fs=float(f[2]), shift=int(w[o + 7]))
        return dict(asym_colour=bool(w[_MODE] & ASYM_COLOUR), asym_rot=bool(w[_MODE] & ASYM_ROLL), r1=int(w[_R1]), r2=int(w[_R2]),
                    rects=[tuple(int(v) for v in w[_RECT + 4 * k:_RECT + 4 * k + 4]) for k in range(int(w[_NRECT]))],
                    set_a=cset(_SET_A), set_b=cset(_SET_B))

    def validate(self, H: int, W: int):
        """Host check of a table (array operations over the rows, no per-row Python).  ``sample_params_360`` fills valid tables
        by construction; the kernels do not trust a table either way."""
        w = self.words
        n = w[:, _NRECT]
        if ((n < 0) | (n > 2)).any():
            raise PfError("AugmentParams: a row with other than 0, 1 or 2 rectangles")
        r = w[:, _RECT:_RECT + 8].reshape(self.B, 2, 4)
        used = np.arange(2)[None, :] < n[:, None]
        bad = used & ~((r[..., 0] >= 0) & (r[..., 0] < W) & (r[..., 1] >= 0) & (r[..., 1] < H) & (r[..., 2] > 0) & (r[..., 3] > 0))
        if bad.any():
            b, k = (int(v) for v in np.argwhere(bad)[0])
            raise PfError(f"AugmentParams: rectangle {tuple(int(v) for v in r[b, k])} of row {b} does not start inside {H}x{W}")
        if (np.abs(w[:, [_R1, _R2]].astype(np.int64)) >= W).any():
            raise PfError(f"AugmentParams: a roll of a whole width ({W}) or more")
        sym = (w[:, _MODE] & ASYM_ROLL) == 0
        if (w[sym, _R1] != w[sym, _R2]).any():
            raise PfError("AugmentParams: r1 != r2 without the asymmetric-roll bit")
        return self

    def equal(self, other: "AugmentParams") -> bool:
        return np.array_equal(self.words, other.words)


_PROBABILITIES = dict(asymmetric_color_aug_prob=0.2, eraser_aug_prob=0.5, rotaton_aug_prob=0.5, asymmetric_rotaton_aug_prob=0.0,
                      rotate_ratio=0.2)


def sample_params_360(B: int, H: int, W: int, rng: np.random.RandomState, gen: torch.Generator,
                      out: Optional[AugmentParams] = None, **probabilities) -> AugmentParams:
    """Draw the augmentation of B samples of H x W on the host, as FlowAugmentor_360 draws them (augmentor.py:220-283; the
    keyword names are its attributes, spelling included): from ``rng`` in the reference's order -- rand (asymmetric colour?),
    rand (eraser?) -> randint(1, 3) -> per rectangle randint(0, W), randint(0, H), randint(50, 100) twice, rand (roll?) ->
    rand (asymmetric?) -> one or two randint(-max, max) -- and the ColorJitter parameters from ``gen`` in torchvision's order:
    randperm(4), then brightness, contrast, saturation, hue as ``uniform_`` of one element each (one set per sample, two for an
    asymmetric one).  ``RandomState(s)`` with ``Generator().manual_seed(s)`` reproduces ``np.random.seed(s);
    torch.manual_seed(s)`` on the reference for one sample.  ``do_flip=True`` or a ``resize_size`` raise PfError."""
    if probabilities.pop("do_flip", False) or probabilities.pop("resize_size", None) is not None:
        raise PfError("sample_params_360: flip_transform and resize_transform are not built (the reference never calls them)")
    unknown = set(probabilities) - set(_PROBABILITIES)
    if unknown:
        raise PfError(f"sample_params_360: unknown parameters {sorted(unknown)}; known: {sorted(_PROBABILITIES)}")
    p = dict(_PROBABILITIES, **probabilities)
    if out is None:
        out = AugmentParams(B)
    elif out.B != B:
        raise PfError(f"sample_params_360: out has {out.B} rows, B = {B}")
    out.words[:] = 0
    one = torch.empty(1)

    def jitter():
        order = torch.randperm(4, generator=gen).tolist()
        f = [float(one.uniform_(lo, hi, generator=gen)) for lo, hi in (FACTOR_RANGE, FACTOR_RANGE, FACTOR_RANGE, HUE_RANGE)]
        return order, f

    max_rot = int(np.round(p["rotate_ratio"] * W))
    for b in range(B):
        asym = rng.rand() < p["asymmetric_color_aug_prob"]
        out.set_asymmetric_colour(b, asym)
        for second in ((False, True) if asym else (False,)):
            order, f = jitter()
            out.set_colour(b, order, f[0], f[1], f[2], hue=f[3], second=second)
        if not asym:
            out.words[b, _SET_B:_SET_B + 8] = out.words[b, _SET_A:_SET_A + 8]
        rects = []
        if rng.rand() < p["eraser_aug_prob"]:
            for _ in range(rng.randint(1, 3)):
                x0, y0 = rng.randint(0, W), rng.randint(0, H)
                dx, dy = rng.randint(*ERASER_BOUNDS), rng.randint(*ERASER_BOUNDS)
                rects.append((x0, y0, dx, dy))
        out.set_rects(b, rects)
        if rng.rand() < p["rotaton_aug_prob"]:
            if rng.rand() < p["asymmetric_rotaton_aug_prob"]:
                r1 = rng.randint(-max_rot, max_rot)
                out.set_roll(b, r1, rng.randint(-max_rot, max_rot))
            else:
                out.set_roll(b, rng.randint(-max_rot, max_rot))
    return out


class DeviceAugmentor360:
    """The augmentation of B samples of H x W on ``device``, with every buffer allocated here: a call launches on the current
    stream, allocates nothing, never synchronises and can be captured into a HIP graph.

    ``__call__(img1_u8 [B,H,W,3], img2_u8 [B,H,W,3], flow [B,H,W,2] fp32, params, out=None)`` ->
    ``(image1 [B,3,H,W], image2, flow_gt [B,2,H,W], valid [B,H,W])``, fp32 device tensors: the augmentor's own (overwritten by
    the next call) or the four given as ``out`` -- e.g. the tensors a ``GraphedTrainStep`` is fed from.  ``params`` is an
    ``AugmentParams`` (validated on the host unless ``validate=False``, then uploaded to ``self.params`` on the current stream; pinned tables upload asynchronously
    and must stay unchanged until that copy has run) or None: the table is ``self.params`` as it stands on the device, which is
    how a captured call is replayed with new parameters (``upload`` them before the replay).
    """

    def __init__(self, B: int, H: int, W: int, device, outputs: bool = True):
        device = torch.device(device)
        if device.type != "cuda":
            raise PfError("DeviceAugmentor360 needs a cuda/ROCm device; there is no CPU fallback")
        if B < 1 or H < 2 or W < 2:
            raise PfError(f"DeviceAugmentor360: B, H, W = {B}, {H}, {W}")
        self.lib = lib = _lib.load()
        self.B, self.H, self.W, self.device = B, H, W, device
        self.params = torch.zeros(B, ROW, dtype=torch.int32, device=device)
        self.scratch = torch.zeros((lib.augment_scratch_bytes(B) + 7) // 8, dtype=torch.int64, device=device)
        self.out = self.new_outputs() if outputs else None

    def new_outputs(self):
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=self.device)  # noqa: E731
        return z(self.B, 3, self.H, self.W), z(self.B, 3, self.H, self.W), z(self.B, 2, self.H, self.W), z(self.B, self.H, self.W)

    def _fit(self, t, shape, what: str, dtype=torch.float32):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise PfError(f"DeviceAugmentor360: {what} must be a device tensor; CPU inputs are refused (there is no CPU fallback)")
        if t.dtype != dtype or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
            raise PfError(f"DeviceAugmentor360: {what} must be a contiguous {dtype} tensor {tuple(shape)}, got {t.dtype} "
                          f"{tuple(t.shape)}")
        return t

    def upload(self, params: AugmentParams, validate: bool = True):
        if not isinstance(params, AugmentParams) or params.B != self.B:
            raise PfError(f"DeviceAugmentor360: params must be an AugmentParams of {self.B} rows")
        if validate:                                        # a table straight from sample_params_360 needs no check
            params.validate(self.H, self.W)
        self.params.copy_(params.table, non_blocking=True)

    def __call__(self, img1_u8, img2_u8, flow, params: Optional[AugmentParams] = None, out=None, validate: bool = True):
        B, H, W = self.B, self.H, self.W
        self._fit(img1_u8, (B, H, W, 3), "img1", torch.uint8)
        self._fit(img2_u8, (B, H, W, 3), "img2", torch.uint8)
        self._fit(flow, (B, H, W, 2), "flow")
        if out is None:
            out = self.out
            if out is None:
                raise PfError("DeviceAugmentor360 was built without outputs: pass out=(image1, image2, flow_gt, valid)")
        elif len(out) != 4:
            raise PfError("DeviceAugmentor360: out is (image1, image2, flow_gt, valid)")
        for t, shape, what in zip(out, ((B, 3, H, W), (B, 3, H, W), (B, 2, H, W), (B, H, W)), ("image1", "image2", "flow_gt", "valid")):
            self._fit(t, shape, "out " + what)
        with torch.cuda.device(self.device):
            if params is not None:
                self.upload(params, validate)
            self.lib.augment_360(img1_u8, img2_u8, flow, self.params, out[0], out[1], out[2], out[3], self.scratch)
        return tuple(out)


def _host(t, dtype, shape, what):
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(t)
    if not isinstance(t, torch.Tensor) or t.is_cuda or t.dtype != dtype or tuple(t.shape) != tuple(shape):
        raise PfError(f"augmented_batches: {what} must be a host {dtype} batch {tuple(shape)}")
    return t.contiguous()


def augmented_batches(loader: Iterable, augmentor: DeviceAugmentor360, rng: np.random.RandomState, gen: torch.Generator,
                      depth: int = 2, **probabilities):
    """Feed a training loop from a loader that does NO augmentation: for each ``(img1_u8 [B,H,W,3], img2_u8, flow [B,H,W,2])``
    host batch of ``loader`` (tensors or numpy arrays; further items of the tuple are ignored) yields ``(image1, image2, flow_gt,
    valid)`` on the device, augmented with ``sample_params_360(B, H, W, rng, gen, **probabilities)`` in loader order.

    The batch is copied from pinned memory and augmented on a side stream into one of ``depth`` output sets; the set is handed to
    the consumer's current stream with an event, so batch i + 1 is prepared while the consumer's step i runs.

    Contract (narrower than "until the batch after the next": with two sets, a set that stayed the consumer's while step i + 1 is
    enqueued could only be refilled behind that step, and nothing would overlap): **the tensors of a yield belong to the consumer
    until it asks for the next batch.**  It may read and overwrite them in place with work enqueued on its current stream up to
    that moment; that work is waited for on the device (an event) before the set is written again, so no host synchronise is
    needed between batches.  After asking for the next batch the consumer must not touch the earlier set again.

    Ordering at the ends: the side stream starts behind everything already queued on the current stream (the buffers are
    allocated there), and when the generator ends -- exhausted, closed, or by an exception -- both streams are synchronised
    before its buffers go back to the allocator, so batches prepared ahead of a ``break`` cannot land in memory given to someone
    else.  Host cost per batch: one ``sample_params_360``, one copy of the batch into pinned memory, and a wait for the event of
    the batch that used this set's pinned buffers ``depth`` batches ago (long done unless the host runs ``depth`` batches ahead of
    the device).  ``train_step`` / ``GraphedTrainStep`` are not involved: hand them the yielded tensors."""
    if depth < 1:
        raise PfError(f"augmented_batches: depth = {depth}")
    a = augmentor
    B, H, W, dev = a.B, a.H, a.W, a.device
    side = torch.cuda.Stream(device=dev)
    pin = lambda shape, dt: torch.empty(shape, dtype=dt, pin_memory=True)  # noqa: E731
    sets = [dict(host=(pin((B, H, W, 3), torch.uint8), pin((B, H, W, 3), torch.uint8), pin((B, H, W, 2), torch.float32)),
                 params=AugmentParams(B, pin=True), out=a.new_outputs(), ready=torch.cuda.Event(), taken=None) for _ in range(depth)]
    dev_in = (torch.empty(B, H, W, 3, dtype=torch.uint8, device=dev), torch.empty(B, H, W, 3, dtype=torch.uint8, device=dev),
              torch.empty(B, H, W, 2, dtype=torch.float32, device=dev))
    # the buffers above (and the augmentor's) were allocated, and the outputs zero-filled, on the current stream: their blocks may
    # still have readers queued there, and the fills must not land after the side stream's first write
    side.wait_stream(torch.cuda.current_stream(dev))

    def prepare(s, batch, first_use):
        i1, i2, fl = (_host(t, dt, sh, w) for t, dt, sh, w in zip(batch[:3], (torch.uint8, torch.uint8, torch.float32),
                                                                    ((B, H, W, 3), (B, H, W, 3), (B, H, W, 2)), ("img1", "img2", "flow")))
        if not first_use:
            s["ready"].synchronize()                        # the copies out of this set's pinned buffers have run
        for dst, src in zip(s["host"], (i1, i2, fl)):
            dst.copy_(src)
        sample_params_360(B, H, W, rng, gen, out=s["params"], **probabilities)
        with torch.cuda.stream(side):
            if s["taken"] is not None:
                side.wait_event(s["taken"])                 # the consumer's work on this set
            for dst, src in zip(dev_in, s["host"]):
                dst.copy_(src, non_blocking=True)
            a(dev_in[0], dev_in[1], dev_in[2], s["params"], out=s["out"], validate=False)
            s["ready"].record(side)

    def give(s):
        cur = torch.cuda.current_stream(dev)
        cur.wait_event(s["ready"])
        yield s["out"]
        s["taken"] = torch.cuda.Event()
        s["taken"].record(torch.cuda.current_stream(dev))

    queue, n = [], 0
    try:
        for batch in loader:
            if len(queue) == depth:                         # every set holds a prepared batch: hand the oldest over first
                yield from give(queue.pop(0))
            s = sets[n % depth]
            prepare(s, batch, n < depth)
            queue.append(s)
            n += 1
        while queue:
            yield from give(queue.pop(0))
    finally:
        # exhausted, closed (a `break` in the consumer's loop) or failed: batches prepared ahead may still be queued on the side
        # stream and the consumer's last reads on its own; both finish before the buffers go back to the allocator
        side.synchronize()
        torch.cuda.current_stream(dev).synchronize()
