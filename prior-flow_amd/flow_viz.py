"""Rendering of panoramic flow on the device: colour coding and the cyclic warp.

The reference's ``core/utils/flow_viz.py`` (``omniflow_to_image``, ``flow_to_image``) and ``core/utils/my_cycle_sample.py``
(``my_cycle_warp``) with the same names and argument order, device tensors in and out: the percentile clip is an exact order
statistic computed on the device (``pf_order_stat``), so nothing is read back and every call can sit behind a ``FlowStream``
step on the same stream or inside the same captured graph.  ``FlowRenderer`` owns the buffers for that.

Not built: ``clip_flow`` (the reference's clamp to [0, clip] zeroes negative components; nobody calls it), ``better_flow_to_image``,
``save_gif`` and its text overlay, and the legacy zero-padded ``warp`` / ``cycle_warp`` of ``core/utils/warp.py``.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from ._lib import PfError


def _flow4(flow: torch.Tensor, what: str) -> torch.Tensor:
    if not isinstance(flow, torch.Tensor) or not flow.is_cuda:
        raise PfError(f"{what} runs on the device; CPU inputs are refused (there is no CPU fallback)")
    if flow.dim() not in (3, 4) or flow.shape[-3] != 2:
        raise PfError(f"{what}: flow {tuple(flow.shape)}, expected planar [2,H,W] or [B,2,H,W]")
    return flow.detach().float().contiguous().view(-1, 2, *flow.shape[-2:])


class FlowRenderer:
    """Colour coding and cyclic warp of the flows of B panoramas of H x W, with every buffer allocated here: ``render`` and
    ``warp`` launch on the current stream, allocate nothing, never synchronise, and can be captured into a HIP graph together
    with a ``FlowStream`` step.

    mode "omni": ``omniflow_to_image`` (great-circle length, clipped at ``percentile`` of each image); "plane":
    ``flow_to_image``.  layout "hwc": images [B,H,W,3] (what an encoder or ``PIL.Image.fromarray`` takes), "chw": [B,3,H,W].
    After ``render``: ``length`` [B,H,W] is the length map and ``clip`` [B] the clip value of each image (views of the scratch).
    """

    def __init__(self, B: int, H: int, W: int, device, mode: str = "omni", percentile: float = 0.95, layout: str = "hwc",
                 bgr: bool = False):
        device = torch.device(device)
        if device.type != "cuda":
            raise PfError("FlowRenderer needs a cuda/ROCm device; there is no CPU fallback")
        self.lib = lib = _lib.load()
        if mode not in lib.RENDER_MODES or layout not in lib.RENDER_LAYOUTS:
            raise PfError(f"FlowRenderer: mode {mode!r} / layout {layout!r}, expected 'omni' | 'plane' and 'hwc' | 'chw'")
        if not 0.0 <= float(percentile) <= 1.0:
            raise PfError(f"FlowRenderer: percentile {percentile!r} outside [0, 1]")
        self.B, self.H, self.W, self.device = B, H, W, device
        self.mode, self.percentile, self.layout, self.bgr = mode, float(percentile), layout, bool(bgr)
        nbytes = lib.flow_render_scratch_bytes(B, H, W)
        self.scratch = torch.zeros((nbytes + 3) // 4, dtype=torch.int32, device=device)
        f = self.scratch.view(torch.float32)
        self.length = f[:B * H * W].view(B, H, W)
        self.clip = f[B * H * W:B * H * W + B]
        self.image = torch.zeros((B, H, W, 3) if layout == "hwc" else (B, 3, H, W), dtype=torch.uint8, device=device)
        self.err = torch.zeros(B, H, W, dtype=torch.float32, device=device)
        self.mean_err = torch.zeros(B, dtype=torch.float32, device=device)
        self.mm_scratch = torch.zeros(128 * B, dtype=torch.float64, device=device)
        self._warped = {}               # channels -> [B,C,H,W], allocated by prepare_warp (or the first warp of that C)

    def _fit(self, t: torch.Tensor, shape, what: str, dtype=torch.float32) -> torch.Tensor:
        if not t.is_cuda or t.dtype != dtype or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
            raise PfError(f"FlowRenderer: {what} must be a contiguous {dtype} device tensor {tuple(shape)}, got {t.dtype} "
                          f"{tuple(t.shape)} on {t.device}")
        return t

    def render(self, flow: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """flow [B,2,H,W] fp32 -> the colour image (``self.image``, or ``out`` of the same shape and dtype)."""
        self._fit(flow, (self.B, 2, self.H, self.W), "flow")
        out = self.image if out is None else self._fit(out, self.image.shape, "out", torch.uint8)
        with torch.cuda.device(self.device):
            self.lib.flow_render(flow, out, self.scratch, self.mode, self.percentile, self.layout, self.bgr)
        return out

    def prepare_warp(self, C: int) -> torch.Tensor:
        """Allocate the output of ``warp`` for C-channel images (do this before capturing a graph that warps)."""
        if C not in self._warped:
            self._warped[C] = torch.zeros(self.B, C, self.H, self.W, dtype=torch.float32, device=self.device)
        return self._warped[C]

    def warp(self, image2: torch.Tensor, flow: torch.Tensor, image1: Optional[torch.Tensor] = None,
             occ: Optional[torch.Tensor] = None):
        """Reconstruct frame 1 from frame 2: ``my_cycle_warp(image2, flow)`` -> (warped, err, mean_err).  With ``image1``:
        err [B,H,W] = mean over channels of |image1 - warped| and mean_err [B] = its mean over the pixels with ``occ == 0``
        (uint8 [B,H,W], e.g. ``occ_forward`` of a bidirectional stream; None: all pixels; 0 when every pixel is occluded),
        both device tensors; without ``image1`` they are None."""
        if image2.dim() != 4:
            raise PfError(f"FlowRenderer.warp: image2 {tuple(image2.shape)}, expected [B,C,H,W]")
        C = image2.shape[1]
        self._fit(image2, (self.B, C, self.H, self.W), "image2")
        self._fit(flow, (self.B, 2, self.H, self.W), "flow")
        if image1 is None and occ is not None:
            raise PfError("FlowRenderer.warp: occ needs image1")
        warped = self.prepare_warp(C)
        with torch.cuda.device(self.device):
            if image1 is None:
                self.lib.cycle_warp(image2, flow, warped)
                return warped, None, None
            self._fit(image1, image2.shape, "image1")
            if occ is not None:
                self._fit(occ, (self.B, self.H, self.W), "occ", torch.uint8)
            self.lib.cycle_warp(image2, flow, warped, ref=image1, err=self.err)
            self.lib.masked_mean(self.err, occ, self.mean_err, self.mm_scratch)
        return warped, self.err, self.mean_err


def _to_image(flow, clip_flow, convert_to_bgr, mode: str, what: str) -> torch.Tensor:
    if clip_flow is not None:
        raise PfError(f"{what}: clip_flow is not supported (the reference's clamp to [0, clip] zeroes negative components)")
    f = _flow4(flow, what)
    B, _, H, W = f.shape
    with torch.no_grad():
        img = FlowRenderer(B, H, W, f.device, mode=mode, bgr=bool(convert_to_bgr)).render(f)
    return img[0] if flow.dim() == 3 else img


def omniflow_to_image(flow_tensor: torch.Tensor, clip_flow=None, convert_to_bgr: bool = False) -> torch.Tensor:
    """The reference's ``omniflow_to_image``: planar flow [2,H,W] -> uint8 [H,W,3] (batched [B,2,H,W] -> [B,H,W,3], each image
    with its own clip), a device tensor.  Colour = direction on the Middlebury wheel, saturation = great-circle length of
    the flow clipped at its 95th percentile.  ``clip_flow`` other than None raises PfError."""
    return _to_image(flow_tensor, clip_flow, convert_to_bgr, "omni", "omniflow_to_image")


def flow_to_image(flow: torch.Tensor, clip_flow=None, convert_to_bgr: bool = False) -> torch.Tensor:
    """The reference's ``flow_to_image`` (saturation = |flow| / max |flow|).  NOTE the layout: the flow is PLANAR here,
    [2,H,W] or [B,2,H,W] as everywhere in this package, not the reference's numpy [H,W,2]; -> uint8 [H,W,3] / [B,H,W,3]."""
    return _to_image(flow, clip_flow, convert_to_bgr, "plane", "flow_to_image")


def my_cycle_warp(x: torch.Tensor, flo: torch.Tensor) -> torch.Tensor:
    """The reference's ``my_cycle_warp``: x [B,C,H,W] sampled at pixel + flo [B,2,H,W] (x wraps, y clamps) -> [B,C,H,W] fp32."""
    if not (isinstance(x, torch.Tensor) and isinstance(flo, torch.Tensor) and x.is_cuda and flo.is_cuda):
        raise PfError("my_cycle_warp runs on the device; CPU inputs are refused (there is no CPU fallback)")
    if x.dim() != 4 or flo.dim() != 4 or flo.shape[1] != 2 or flo.shape[0] != x.shape[0] or flo.shape[2:] != x.shape[2:]:
        raise PfError(f"my_cycle_warp: x {tuple(x.shape)} / flo {tuple(flo.shape)}, expected [B,C,H,W] and [B,2,H,W]")
    with torch.no_grad(), torch.cuda.device(x.device):
        xs, fs = x.detach().float().contiguous(), flo.detach().float().contiguous()
        return _lib.load().cycle_warp(xs, fs, torch.empty_like(xs))
