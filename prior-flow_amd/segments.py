"""Moving objects on the device: connected components of a byte mask on the cyclic panorama, per-component sums and a dense,
capped object table.

    objects = MovingObjects(B, H, W, device, channels=3)
    ids, count, table = objects.update_parallax(odo.map_b[3], flow, prop.rigid_flow, prop.inv_depth)
    table[b, k]            # object k + 1 of image b: area, pixels, centroid x, y, resultant length, value weight, mean u, v, 1/depth
    objects.keep           # the mask without its small components: what PoseEstimator and ScaleLink want as a mask

A pixel is set when its byte is non-zero.  Column W-1 touches column 0; with ``poles`` the set pixels of row 0 are one component
(they meet at the pole) and so are those of row H-1.  The label of a set pixel is 1 + the smallest linear index y W + x of its
component, so the labels are a function of the mask alone.  Components whose cos-latitude-weighted area reaches ``min_area``
(pixels at the equator) survive and are numbered 1, 2, ... by that smallest index; those beyond ``max_objects`` get id 0 but stay
in ``keep``, and ``count`` is not clipped, so an overflow shows.  There is no CPU path: tensors on the host are refused (PfError).

min_area = 4.0 and max_objects = 64 are choices, not measurements.
"""
from __future__ import annotations

import math

import torch

from ._lib import SEG_COLS, SEG_MAX_OBJECTS, SEG_SUMS, PfError
from .egomotion import _device, _fit, _library, _on

TABLE_COLUMNS = ("area", "pixels", "x", "y", "resultant", "value_weight")


def _geometry(what, connectivity, poles):
    if connectivity not in (4, 8):
        raise PfError(f"{what}: connectivity = {connectivity!r}, expected 4 or 8")
    if poles not in (False, True, 0, 1):
        raise PfError(f"{what}: poles = {poles!r}, expected a bool")


class _Tables:
    """rows [H,2], cols [W,2] and the scratch of one geometry."""

    def __init__(self, B, H, W, device, lib):
        self.rows = torch.zeros(H, 2, dtype=torch.float32, device=device)
        self.cols = torch.zeros(W, 2, dtype=torch.float32, device=device)
        self.scratch = torch.zeros(lib.seg_scratch_bytes(B, H, W) // 8, dtype=torch.int64, device=device)
        with _on(device):
            lib.seg_tables(self.rows, self.cols)


def label_components(mask, connectivity: int = 8, poles: bool = False, out=None, lib=None):
    """labels int32 [B,H,W] of mask uint8 [B,H,W]: 1 + the smallest linear index of the pixel's component, 0 for background.
    The buffers are allocated per call (for a video use ``MovingObjects``)."""
    if not isinstance(mask, torch.Tensor) or mask.dim() != 3:
        raise PfError("label_components: mask must be a tensor [B,H,W]")
    B, H, W = mask.shape
    dev = mask.device
    lib = _library(dev, lib)
    _fit(mask, (B, H, W), "label_components: mask", dev, torch.uint8)
    _geometry("label_components", connectivity, poles)
    if out is None:
        out = torch.empty(B, H, W, dtype=torch.int32, device=dev)
    else:
        _fit(out, (B, H, W), "label_components: out", dev, torch.int32)
    t = _Tables(B, H, W, dev, lib)
    with _on(dev):
        lib.seg_label(mask, t.rows, out, t.scratch, connectivity, bool(poles))
    return out


class MovingObjects:
    """The objects of B masks [H,W], with every buffer allocated here: ``update`` launches eight kernels on the current stream
    (label: tiles, merge, flatten; objects: count, scan, assign, accumulate, resolve), allocates nothing, never synchronises,
    reads nothing on the host and can be captured into a HIP graph.  Nothing it computes depends on what its buffers held before.

    ``table`` [B, max_objects, 6 + channels]: area (pixels at the equator), pixels, centroid x, y (ERP pixels, of the summed
    bearing), resultant length (near 1 for a compact object, towards 0 for one that wraps the sphere), value weight, then the
    cos-latitude-weighted means of the value channels over the pixels whose values are all below 2^16 in magnitude.  Unused rows
    are zero.  ``ids``, ``count``, ``table``, ``keep``, ``roots``, ``labels`` and ``sums`` stay readable until the next call."""

    def __init__(self, B: int, H: int, W: int, device, max_objects: int = 64, min_area: float = 4.0, connectivity: int = 8,
                 poles: bool = False, channels: int = 0, lib=None):
        self.lib = _library(device, lib)
        self.device = dev = _device(device)
        if min(B, H, W) < 1:
            raise PfError(f"MovingObjects: B, H, W = {B}, {H}, {W}")
        if not isinstance(max_objects, int) or not 1 <= max_objects <= SEG_MAX_OBJECTS:
            raise PfError(f"MovingObjects: max_objects = {max_objects!r}, expected 1..{SEG_MAX_OBJECTS}")
        if channels not in (0, 1, 2, 3, 4):
            raise PfError(f"MovingObjects: channels = {channels!r}, expected 0..4")
        try:
            min_area = float(min_area)
        except (TypeError, ValueError):
            raise PfError(f"MovingObjects: min_area = {min_area!r}") from None
        if not (math.isfinite(min_area) and 0 <= min_area <= 2.0 ** 30):
            raise PfError(f"MovingObjects: min_area = {min_area!r}, expected 0..2^30")
        _geometry("MovingObjects", connectivity, poles)
        self.B, self.H, self.W, self.M, self.C = B, H, W, max_objects, int(channels)
        self.min_area, self.connectivity, self.poles = min_area, connectivity, bool(poles)
        self._t = _Tables(B, H, W, dev, self.lib)
        i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)                      # noqa: E731
        self.labels, self.ids, self.roots, self.count = i32(B, H, W), i32(B, H, W), i32(B, max_objects), i32(B)
        self.keep = torch.zeros(B, H, W, dtype=torch.uint8, device=dev)
        self.table = torch.zeros(B, max_objects, SEG_COLS + self.C, dtype=torch.float32, device=dev)
        self.sums = torch.zeros(B, max_objects, SEG_SUMS, dtype=torch.int64, device=dev)
        self.values = torch.zeros(B, self.C, H, W, dtype=torch.float32, device=dev) if self.C else None

    @property
    def rows(self):
        return self._t.rows

    @property
    def cols(self):
        return self._t.cols

    def update(self, mask, values=None):
        """(ids int32 [B,H,W], count int32 [B], table fp32 [B,M,6+C]) of mask uint8 [B,H,W]; values fp32 [B,C,H,W] (None when
        channels = 0)."""
        B, H, W, C, dev = self.B, self.H, self.W, self.C, self.device
        _fit(mask, (B, H, W), "MovingObjects.update: mask", dev, torch.uint8)
        if (values is None) != (C == 0):
            raise PfError(f"MovingObjects.update: values are {'required' if C else 'not taken'} with channels = {C}")
        if values is not None:
            _fit(values, (B, C, H, W), "MovingObjects.update: values", dev)
        mine = {t.data_ptr(): n for n, t in (("labels", self.labels), ("ids", self.ids), ("keep", self.keep), ("table", self.table))}
        for name, t in (("mask", mask), ("values", values)):
            if t is not None and t.data_ptr() in mine and t is not self.values:
                raise PfError(f"MovingObjects.update: {name} aliases {mine[t.data_ptr()]}")
        t = self._t
        with _on(dev):
            self.lib.seg_label(mask, t.rows, self.labels, t.scratch, self.connectivity, self.poles)
            self.lib.seg_objects(self.labels, values, t.rows, t.cols, t.scratch, self.ids, self.keep, self.roots, self.count,
                                 self.table, self.sums, self.min_area)
        return self.ids, self.count, self.table

    def update_parallax(self, moving, flow, rigid_flow, inv_depth):
        """The objects of ``parallax_map``'s moving bytes [B,H,W], described by their independent motion (u, v) = flow - rigid_flow
        (fp32 [B,2,H,W] each; ``DepthPropagator.rigid_flow`` is what depth and pose predict) and their inverse depth fp32 [B,H,W]:
        needs channels = 3; table[..., 6:9] = mean u, v (pixels) and mean inverse depth."""
        B, H, W, dev = self.B, self.H, self.W, self.device
        if self.C != 3:
            raise PfError(f"MovingObjects.update_parallax: needs channels = 3, this object has {self.C}")
        _fit(moving, (B, H, W), "MovingObjects.update_parallax: moving", dev, torch.uint8)
        _fit(flow, (B, 2, H, W), "MovingObjects.update_parallax: flow", dev)
        _fit(rigid_flow, (B, 2, H, W), "MovingObjects.update_parallax: rigid_flow", dev)
        _fit(inv_depth, (B, H, W), "MovingObjects.update_parallax: inv_depth", dev)
        with _on(dev):
            torch.sub(flow, rigid_flow, out=self.values[:, :2])
            self.values[:, 0].add_(W / 2).remainder_(W).sub_(W / 2)        # u is cyclic: the difference of two wrapped flows
            self.values[:, 2].copy_(inv_depth)
        return self.update(moving, self.values)
