"""Self-supervised fine-tuning on unlabelled 360-degree video: a criterion that needs no ground truth, with
its gradient, and the optimisation step that drives it.

  * ``SelfSupervisedLoss(H, W)(flow_preds, image1, image2, mask)`` -> ``(loss, metrics)`` has ``train.uniform_loss``'s shape: a
    spherical photometric term through the model's cyclic sampler (the taps of ``pf_cycle_warp``) plus a first-order edge-aware
    smoothness term, both weighted by solid angle; d loss / d prediction of every prediction is left in ``.grads`` (one
    ``pf_selfsup_loss_batch`` launch per 32 predictions; the statement is ``csrc/pf_selfsup.h``);
  * ``to_view_b(image)`` rotates a frame into branch B's view (``pf_img_rotate`` with the grid the model uses);
  * ``train_step_selfsup(model, optimizer, scheduler, criterion, image1, image2)`` is ``train.train_step`` without ``flow_gt``:
    both orders of the pair in one batch, occlusion masks from the forward-backward check of the two halves.

The default weights are choices, not measurements."""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib, parallel
from .engine import rotation_x
from .evaluate import spherical_mask
from .train import MAX_FLOW, SYNC_CHECK_EVERY, FlatAdamW, OneCycleLinearLR, _grad_sink, clip_grad_norm_
from .video import forward_backward_check


class SelfSupervisedLoss:
    PIXELS_PER_CHUNK = 256          # one pixel per thread of a workgroup
    MAX_NBLK = 1024

    def __init__(self, H: int, W: int, device=None, w_photo: float = 1.0, w_smooth: float = 2.0, eps_photo: float = 0.01,
                 eps_smooth: float = 0.001, edge_lambda: float = 150.0, max_flow: float = MAX_FLOW, lib=None, blocks: int = 0):
        self.lib = _lib.load() if lib is None else lib
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.H, self.W = H, W
        self.w_photo, self.w_smooth, self.eps_photo, self.eps_smooth = float(w_photo), float(w_smooth), float(eps_photo), float(eps_smooth)
        self.edge_lambda, self.max_flow = float(edge_lambda), float(max_flow)
        self.blocks = int(blocks)                                        # workgroups per launch, 0: one per (chunk, image)
        w = torch.from_numpy(spherical_mask(H, W)).float().contiguous()  # H x W, the weight uniform_loss uses
        self.weight_sum = float(w.double().sum())                        # Z = B * this, from the fp32 values the kernel reads
        self.uniform_mask = w.to(self.device)
        self._weights: Dict[str, torch.Tensor] = {str(self.device): self.uniform_mask}      # the weight, once per device
        self.nblk = max(1, min(self.MAX_NBLK, (H * W + self.PIXELS_PER_CHUNK - 1) // self.PIXELS_PER_CHUNK))
        self.grads: List[torch.Tensor] = []
        self._state: Dict[tuple, dict] = {}                              # the buffers of a lazy call, per shape

    def _buffers(self, n, B, dev, gamma, extro_info, need_grads):
        weights = [gamma ** (n - i - 1) for i in range(n)]
        z = B * self.weight_sum
        f64 = dict(dtype=torch.float64, device=dev)
        coef = torch.tensor([[w * self.w_photo, w * self.w_smooth, 0.0, 0.0] for w in weights], **f64)
        return dict(weights=weights, z=z, coef=coef, scale=torch.tensor([1.0, 1.0, 1.0 / z, 1.0], **f64),
                    part=torch.empty(n, B, self.nblk, _lib.SS_SUMS, **f64), tot=torch.empty(n, _lib.SS_SUMS, **f64),
                    tmp=torch.empty(n, _lib.SS_SUMS, **f64), loss64=torch.empty((), **f64), loss=torch.empty((), device=dev),
                    met=torch.empty(_lib.SS_SUMS, **f64),
                    grads=[torch.empty(B, 2, self.H, self.W, device=dev) for _ in range(n)] if need_grads else [])

    @torch.no_grad()
    def __call__(self, flow_preds: Sequence[torch.Tensor], image1: torch.Tensor, image2: torch.Tensor,
                 mask: Optional[torch.Tensor] = None, gamma: float = 0.8, extro_info: str = "", need_grads: bool = True,
                 lazy: bool = False) -> Tuple[torch.Tensor, Dict[str, float]]:
        """flow_preds: the predictions of one branch, [B,2,H,W] each; image1, image2 [B,3,H,W] in 0..255 in that branch's view; mask
        uint8 [B,H,W] or None (non-zero: the pixel's photometric term is left out).  metrics: ``photo`` and ``smooth`` of the last
        prediction, ``used`` (the share of the solid angle its photometric term covered) and ``left_out`` (its flows that were not
        finite or out of range).

        lazy: nothing is read on the host, and after the first call of a (shape, extro_info) nothing is allocated: loss, metrics
        and ``.grads`` are that state's own tensors, which its next lazy call overwrites.  Capturable (call once before the
        capture)."""
        n = len(flow_preds)
        if n < 1:
            raise _lib.PfError("SelfSupervisedLoss: no predictions")
        i1, i2 = image1.float().contiguous(), image2.float().contiguous()
        B, dev = i1.shape[0], i1.device
        if tuple(i1.shape[1:]) != (3, self.H, self.W):
            raise _lib.PfError(f"SelfSupervisedLoss({self.H}, {self.W}): image1 is {tuple(i1.shape)}")
        if mask is not None and mask.dtype != torch.uint8:
            mask = (mask != 0).to(torch.uint8)
        preds = [p.detach().float().contiguous() for p in flow_preds]
        key = (n, B, str(dev), float(gamma), extro_info, bool(need_grads))
        st = self._state.get(key) if lazy else None
        if st is None:
            st = self._buffers(n, B, dev, gamma, extro_info, need_grads)
            if lazy:
                self._state[key] = st
        self.grads = st["grads"]
        weight = self._weights.get(str(dev))
        if weight is None:                                               # a device the constructor was not told of: copied once
            weight = self._weights[str(dev)] = self.uniform_mask.to(dev)
        for lo in range(0, n, _lib.SS_MAX):                              # 32 terms per launch
            hi = min(n, lo + _lib.SS_MAX)
            self.lib.selfsup_loss_batch(preds[lo:hi], i1, i2, weight.view(-1), mask, st["weights"][lo:hi],
                                        st["grads"][lo:hi] if need_grads else None, st["part"][lo:hi], st["z"], self.w_photo,
                                        self.w_smooth, self.eps_photo, self.eps_smooth, self.edge_lambda, self.max_flow,
                                        blocks=self.blocks)
        torch.sum(st["part"], dim=(1, 2), out=st["tot"])                 # the chunks, in chunk order: [n, 4]
        torch.mul(st["tot"], st["coef"], out=st["tmp"])
        torch.sum(st["tmp"], dim=(0, 1), out=st["loss64"])
        st["loss"].copy_(st["loss64"])
        torch.mul(st["tot"][-1], st["scale"], out=st["met"])
        names = ("photo", "smooth", "used", "left_out")
        if lazy:
            return st["loss"], {extro_info + k: st["met"][j] for j, k in enumerate(names)}
        return st["loss"], {extro_info + k: v for k, v in zip(names, st["met"].tolist())}


_VIEW_GRIDS: Dict[tuple, torch.Tensor] = {}


@torch.no_grad()
def to_view_b(image: torch.Tensor) -> torch.Tensor:
    """A frame [B,3,H,W] in branch B's view: img_rotate with grid(R_A2B), R_A2B = Rx(-pi / 2) (core/prior_raft.py:115-125), what
    the model does to its inputs.  The grid is built once per (H, W, device)."""
    lib = _lib.load()
    img = image.float().contiguous()
    _, _, H, W = img.shape
    key = (H, W, str(img.device))
    if key not in _VIEW_GRIDS:
        _VIEW_GRIDS[key] = lib.sample_grid(torch.empty(2, H, W, device=img.device), rotation_x(-math.pi / 2))
    return lib.img_rotate(img, _VIEW_GRIDS[key], torch.empty_like(img))


@torch.no_grad()
def occlusion_masks(final_pred: torch.Tensor, occlusion: str = "fb") -> torch.Tensor:
    """uint8 [2B,H,W] for a batch [first; second] -> [second; first]: "fb": pair j gets occ_fw and pair B + j occ_bw of
    forward_backward_check(final_pred[:B], final_pred[B:], metric="sphere"); "none": zeros."""
    f = final_pred.detach().float().contiguous()
    B2, _, H, W = f.shape
    if occlusion == "none":
        return torch.zeros(B2, H, W, dtype=torch.uint8, device=f.device)
    if occlusion != "fb":
        raise _lib.PfError(f"occlusion must be 'fb' or 'none', not {occlusion!r}")
    occ_fw, occ_bw, _, _ = forward_backward_check(f[:B2 // 2], f[B2 // 2:], metric="sphere")
    return torch.cat([occ_fw, occ_bw])


def train_step_selfsup(model, optimizer: FlatAdamW, scheduler: OneCycleLinearLR, criterion: SelfSupervisedLoss,
                       image1: torch.Tensor, image2: torch.Tensor, iters: int = 12, gamma: float = 0.8, clip: float = 1.0,
                       group=None, occlusion: str = "fb"):
    """One optimisation step on an unlabelled pair of consecutive frames [B,3,H,W] (0..255): ``train.train_step`` with
    ``SelfSupervisedLoss`` in the place of the sequence loss.  The batch is both orders of the pair, [image1; image2] ->
    [image2; image1], 2B pairs, each trained; with ``occlusion="fb"`` the photometric masks of pair j and pair B + j are occ_fw /
    occ_bw of ``forward_backward_check`` on the detached final predictions' two halves, per branch, so occlusion costs no forward
    of its own.  Branch B's criterion sees both frames through ``to_view_b``.  Returns ``(loss, metrics)``;
    ``metrics['grad_norm']`` is the pre-clip total norm."""
    if occlusion not in ("fb", "none"):
        raise _lib.PfError(f"occlusion must be 'fb' or 'none', not {occlusion!r}")
    net = getattr(model, "module", model)
    optimizer.zero_grad()
    with torch.no_grad():
        first = torch.cat([image1, image2]).float().contiguous()
        second = torch.cat([image2, image1]).float().contiguous()
        first_b, second_b = to_view_b(first), to_view_b(second)
    sink = _grad_sink(optimizer)
    try:
        preds_a, preds_b = net(first, second, iters=iters)
        loss_a, metrics_a = criterion(preds_a, first, second, occlusion_masks(preds_a[-1], occlusion), gamma, extro_info="A-")
        seeds = list(criterion.grads)
        loss_b, metrics_b = criterion(preds_b, first_b, second_b, occlusion_masks(preds_b[-1], occlusion), gamma, extro_info="B-")
        seeds += list(criterion.grads)
        torch.autograd.backward(list(preds_a) + list(preds_b), seeds)
    except BaseException:
        sink.abort()            # nothing half-accumulated is added to the gradients; the sink is off for whoever runs next
        raise
    sink.flush()
    parallel.all_reduce_sum_(optimizer.grad, group)
    norm = clip_grad_norm_(optimizer, clip)
    optimizer.step()
    scheduler.step()
    if optimizer.step_count % SYNC_CHECK_EVERY == 1:
        optimizer.assert_in_sync(group)
    return loss_a + loss_b, {**metrics_a, **metrics_b, "grad_norm": norm}
