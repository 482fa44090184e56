"""Perspective viewports and cube maps of panoramic frames and flow on the device.

Everything the model delivers is an equirectangular (ERP) map.  ``ViewRenderer`` turns frames, rendered flow images and the flow
itself into pinhole views -- a player's viewport, the six faces of a cube map, the input of ordinary perspective code -- with the
reference's pixel-centre and axis conventions (``core/utils/projection_prim_ortho.py:264-430``) stated once, in
``csrc/pf_viewport.h``.  The flow is not resampled channel by channel: the 3-D displacement of the end point is interpolated and
projected through the camera (``pf_viewport_flow``), so the seam and the poles need no special case.

Not built: flow from cube faces back to ERP, fisheye models, backward passes, filtering across face edges, anti-aliasing (a view
coarser than the panorama is point-sampled with four taps).
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import torch

from . import _lib
from ._lib import PfError

MIN_FORWARD = math.cos(math.radians(85.0))


def rotation(yaw: float, pitch: float, roll: float):
    """R = Rz(yaw) Ry(pitch) Rx(roll), the reference's ``generate_rotation_metrix(theta_list=[yaw, pitch, roll])``, as three rows
    (float64).  Columns: forward, right, up in world axes; a positive pitch looks towards -z (down: +n)."""
    cz, sz, cy, sy, cx, sx = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch), math.cos(roll), math.sin(roll)
    rz = ((cz, -sz, 0.0), (sz, cz, 0.0), (0.0, 0.0, 1.0))
    ry = ((cy, 0.0, sy), (0.0, 1.0, 0.0), (-sy, 0.0, cy))
    rx = ((1.0, 0.0, 0.0), (0.0, cx, -sx), (0.0, sx, cx))
    mul = lambda a, b: tuple(tuple(sum(a[i][k] * b[k][j] for k in range(3)) for j in range(3)) for i in range(3))  # noqa: E731
    return mul(mul(rz, ry), rx)


class View:
    """A pinhole view (R, f, h, w): R 3x3 with columns forward, right, up in world axes, f the focal length in pixels, the
    principal point at ((w - 1) / 2, (h - 1) / 2)."""

    def __init__(self, R, f: float, h: int, w: int):
        self.R = tuple(tuple(float(v) for v in r) for r in R)
        self.f, self.h, self.w = float(f), int(h), int(w)
        if len(self.R) != 3 or any(len(r) != 3 for r in self.R):
            raise PfError("View: R is 3 x 3")
        if not (math.isfinite(self.f) and self.f > 0.0) or self.h < 1 or self.w < 1:
            raise PfError(f"View: f {f!r} must be positive and finite, h x w {h!r} x {w!r} at least 1 x 1")

    def row(self):
        """The view's row of the C-ABI's table: R row-major, f, h, w."""
        return [v for r in self.R for v in r] + [self.f, float(self.h), float(self.w)]


class Viewport(View):
    """The view of a player or head-set: yaw, pitch, roll in radians (R = Rz(yaw) Ry(pitch) Rx(roll)), horizontal field of view
    in degrees, h x w pixels; f = (w / 2) / tan(fov_x / 2).  All angles zero: the view looks at the ERP centre, right is +m and
    down is +n."""

    def __init__(self, yaw: float, pitch: float, roll: float, fov_x_deg: float, h: int, w: int):
        if not 0.0 < float(fov_x_deg) < 180.0:
            raise PfError(f"Viewport: fov_x_deg {fov_x_deg!r} outside (0, 180)")
        super().__init__(rotation(yaw, pitch, roll), (w / 2.0) / math.tan(math.radians(fov_x_deg) / 2.0), h, w)
        self.yaw, self.pitch, self.roll, self.fov_x_deg = float(yaw), float(pitch), float(roll), float(fov_x_deg)


# columns [forward, right, up] of the six cube faces, in the order of the face axis of a cube map tensor
CUBE_FACES = (("front", (1, 0, 0), (0, 1, 0), (0, 0, 1)), ("right", (0, 1, 0), (-1, 0, 0), (0, 0, 1)),
              ("back", (-1, 0, 0), (0, -1, 0), (0, 0, 1)), ("left", (0, -1, 0), (1, 0, 0), (0, 0, 1)),
              ("up", (0, 0, 1), (0, 1, 0), (-1, 0, 0)), ("down", (0, 0, -1), (0, 1, 0), (1, 0, 0)))


def cube_faces(s: int):
    """The six views of a cube map with faces of s x s pixels (front, right, back, left, up, down; f = s / 2)."""
    return [View([[fw[i], rt[i], up[i]] for i in range(3)], s / 2.0, s, s) for _, fw, rt, up in CUBE_FACES]


class ViewRenderer:
    """V pinhole views of B panoramas of H x W, with every buffer allocated here (or by ``prepare``): ``image`` and ``flow``
    launch on the current stream, allocate nothing, never synchronise, and can be captured into a HIP graph together with a
    ``FlowStream`` step and a ``FlowRenderer``.  All views share one size h x w; at most 16 views.

    ``image(x)``: fp32 frames [B,C,H,W] -> [B,V,C,h,w], or uint8 channel-last images [B,H,W,C] (what ``FlowRenderer.render``
    writes) -> [B,V,h,w,C].  ``flow(flow)``: ERP flow [B,2,H,W] -> (pinhole flow [B,V,2,h,w] in view pixels, valid uint8
    [B,V,h,w]); valid is 0 where a tap's flow is not finite or the end point leaves the half space q_f > min_forward |q|
    (default cos 85 deg), and the flow is (0, 0) there."""

    def __init__(self, B: int, H: int, W: int, views: Sequence[View], device, min_forward: float = MIN_FORWARD):
        device = torch.device(device)
        if device.type != "cuda":
            raise PfError("ViewRenderer needs a cuda/ROCm device; there is no CPU fallback")
        views = list(views)
        if not 1 <= len(views) <= _lib.VIEW_MAX or not all(isinstance(v, View) for v in views):
            raise PfError(f"ViewRenderer: 1..{_lib.VIEW_MAX} View objects, got {len(views)}")
        if any((v.h, v.w) != (views[0].h, views[0].w) for v in views):
            raise PfError("ViewRenderer: the views of one renderer share one size h x w")
        if not 0.0 < float(min_forward) < 1.0:
            raise PfError(f"ViewRenderer: min_forward {min_forward!r} outside (0, 1)")
        if B < 1 or H < 1 or W < 1:
            raise PfError(f"ViewRenderer: B, H, W = {B}, {H}, {W}")
        self.lib = _lib.load()
        self.B, self.H, self.W, self.device = B, H, W, device
        self.views, self.V, self.h, self.w = views, len(views), views[0].h, views[0].w
        self.min_forward = float(min_forward)
        self.table = self.lib.view_table([v.row() for v in views])
        self.flow_out = torch.zeros(B, self.V, 2, self.h, self.w, dtype=torch.float32, device=device)
        self.valid = torch.zeros(B, self.V, self.h, self.w, dtype=torch.uint8, device=device)
        self._images = {}               # (channels, dtype) -> output of image(), allocated by prepare (or the first call)

    def _fit(self, t, shape, what: str, dtype) -> torch.Tensor:
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or not t.is_contiguous() \
                or tuple(t.shape) != tuple(shape):
            got = f"{t.dtype} {tuple(t.shape)} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
            raise PfError(f"ViewRenderer: {what} must be a contiguous {dtype} device tensor {tuple(shape)}, got {got}")
        return t

    def _image_shape(self, C: int, dtype):
        return (self.B, self.V, C, self.h, self.w) if dtype == torch.float32 else (self.B, self.V, self.h, self.w, C)

    def prepare(self, C: int, dtype=torch.float32) -> torch.Tensor:
        """Allocate the output of ``image`` for C-channel inputs of ``dtype`` (do this before capturing a graph)."""
        if dtype not in (torch.float32, torch.uint8) or C < 1:
            raise PfError(f"ViewRenderer.prepare: C {C!r}, dtype {dtype!r}; expected C >= 1 and torch.float32 | torch.uint8")
        key = (int(C), dtype)
        if key not in self._images:
            self._images[key] = torch.zeros(self._image_shape(C, dtype), dtype=dtype, device=self.device)
        return self._images[key]

    def image(self, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """fp32 [B,C,H,W] -> [B,V,C,h,w]; uint8 [B,H,W,C] -> [B,V,h,w,C] (rounded to nearest, clamped to 0..255)."""
        if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.dtype not in (torch.float32, torch.uint8):
            raise PfError("ViewRenderer.image: expected fp32 [B,C,H,W] or uint8 [B,H,W,C]")
        C = x.shape[1] if x.dtype == torch.float32 else x.shape[3]
        self._fit(x, (self.B, C, self.H, self.W) if x.dtype == torch.float32 else (self.B, self.H, self.W, C), "x", x.dtype)
        out = self.prepare(C, x.dtype) if out is None else self._fit(out, self._image_shape(C, x.dtype), "out", x.dtype)
        with torch.cuda.device(self.device):
            self.lib.viewport_image(x, self.table, out)
        return out

    def flow(self, flow: torch.Tensor, out: Optional[torch.Tensor] = None):
        """ERP flow [B,2,H,W] fp32 -> (pinhole flow [B,V,2,h,w], valid uint8 [B,V,h,w])."""
        self._fit(flow, (self.B, 2, self.H, self.W), "flow", torch.float32)
        out = self.flow_out if out is None else self._fit(out, self.flow_out.shape, "out", torch.float32)
        with torch.cuda.device(self.device):
            self.lib.viewport_flow(flow, self.table, out, self.valid, self.min_forward)
        return out, self.valid


def _frames(x, what: str, dims: int) -> torch.Tensor:
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise PfError(f"{what} runs on the device; CPU inputs are refused (there is no CPU fallback)")
    if x.dim() != dims or x.dtype != torch.float32:
        raise PfError(f"{what}: {x.dtype} {tuple(x.shape)}, expected an fp32 tensor of {dims} dimensions")
    return x.detach().contiguous()


def erp_to_cubemap(x: torch.Tensor, s: int) -> torch.Tensor:
    """ERP frames [B,C,H,W] fp32 -> cube faces [B,6,C,s,s] (front, right, back, left, up, down)."""
    x = _frames(x, "erp_to_cubemap", 4)
    B, _, H, W = x.shape
    with torch.no_grad():
        return ViewRenderer(B, H, W, cube_faces(s), x.device).image(x)


def cubemap_to_erp(faces: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """Cube faces [B,6,C,s,s] fp32 -> ERP frames [B,C,H,W]; bilinear inside each face, no filtering across face edges."""
    faces = _frames(faces, "cubemap_to_erp", 5)
    if faces.shape[1] != 6 or faces.shape[3] != faces.shape[4] or H < 1 or W < 1:
        raise PfError(f"cubemap_to_erp: faces {tuple(faces.shape)}, expected [B,6,C,s,s]; H x W {H!r} x {W!r}")
    with torch.no_grad(), torch.cuda.device(faces.device):
        out = torch.empty(faces.shape[0], faces.shape[2], H, W, dtype=torch.float32, device=faces.device)
        return _lib.load().cubemap_to_erp(faces, out)
