"""Object tracks on the device: persistent ids for the objects of ``MovingObjects`` across frames, from flow votes (DESIGN.md
section 26).

    objects = MovingObjects(B, H, W, device, channels=3)
    tracker = ObjectTracker(objects)                       # every buffer allocated here
    for r in pairs:                                        # r: a BidirectionalFlow of FlowStream(..., bidirectional=True)
        objects.update_parallax(moving, r.forward, rigid_flow, inv_depth)
        track, age, track_map = tracker.push(r)
    track[b, k]            # the persistent id of object k + 1 of image b; age[b, k] pushes it has lived; track_map the id per pixel
    tracker.origin, tracker.fate, tracker.step, tracker.path, tracker.next_id, tracker.votes

An id of ``MovingObjects`` is the rank of the object's smallest pixel index in ONE frame.  The tracker links the objects of two
consecutive frames: every pixel of an object follows the flow into the other frame and votes, with its cos-latitude area weight,
for the object it lands on; a cell of the vote matrix counts when it reaches ``min_overlap`` of the smaller of the two areas (per
flow that voted); an object continues a track when it and its predecessor are each other's best cell (ties go to the smaller
slot).  ``origin`` names the track a new object split from (0: none), ``fate`` says per previous slot where it went (slot + 1),
into which slot it merged (negative) or that it is lost (0); ``step`` is the great-circle angle in radians its summed bearing moved
by and ``path`` the sum of the steps.  All sums are 64-bit integers, so a push gives the same bits on every run.  There is no CPU
path: tensors on the host are refused (PfError).

min_overlap = 0.25 is a choice, not a measurement.
"""
from __future__ import annotations

import math

import torch

from ._lib import SEG_SUMS, TRK_MAX_OBJECTS, PfError
from .egomotion import _fit, _on
from .segments import MovingObjects


class ObjectTracker:
    """Tracks over the objects of ``objects`` (a ``MovingObjects`` with max_objects <= 256).  ``push`` / ``link`` launch four
    kernels with one flow, five with two (begin, vote per flow, match, paint) on the current stream, allocate nothing, never
    synchronise, read nothing on the host and can be captured into a HIP graph; nothing they compute depends on what an output
    buffer held before.  Call them after ``objects.update*`` of the same frame.

    grid = "first": the masks live on the first frame of each pair (``parallax_map(r.forward, ...)``), so the objects of push
    k + 1 are on frame k's grid and those of push k on frame k - 1's; the flows that link them are pair k's ``forward`` and
    ``backward``, which ``push`` copies (with their occlusion masks) into buffers of its own at the end of push k and uses at
    push k + 1.  grid = "second": the masks live on the later frame (``occ_backward``); the current pair's flows link directly.

    ``track``, ``age``, ``origin`` int32 [B,M] and ``step``, ``path`` fp32 [B,M] describe the current slots (rows beyond
    min(count, M) are zero), ``fate`` int32 [B,M] the previous ones, ``track_map`` int32 [B,H,W] holds the track of each pixel's
    object, ``votes`` int64 [B,M,M] the vote matrix, ``next_id`` int32 [B] the next unused id."""

    def __init__(self, objects: MovingObjects, min_overlap: float = 0.25, grid: str = "first"):
        if not isinstance(objects, MovingObjects):
            raise PfError(f"ObjectTracker: objects must be a MovingObjects, got {type(objects).__name__}")
        if objects.M > TRK_MAX_OBJECTS:
            raise PfError(f"ObjectTracker: objects.max_objects = {objects.M}, expected at most {TRK_MAX_OBJECTS}")
        try:
            min_overlap = float(min_overlap)
        except (TypeError, ValueError):
            raise PfError(f"ObjectTracker: min_overlap = {min_overlap!r}") from None
        if not (math.isfinite(min_overlap) and 0.0 < min_overlap <= 1.0):
            raise PfError(f"ObjectTracker: min_overlap = {min_overlap!r}, expected a value in (0, 1]")
        if grid not in ("first", "second"):
            raise PfError(f"ObjectTracker: grid = {grid!r}, expected 'first' or 'second'")
        self.objects, self.lib, self.device = objects, objects.lib, objects.device
        self.B, self.H, self.W, self.M = objects.B, objects.H, objects.W, objects.M
        self.min_overlap, self.grid = min_overlap, grid
        B, H, W, M, dev = self.B, self.H, self.W, self.M, self.device
        i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)                      # noqa: E731
        f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)                    # noqa: E731
        self.votes = torch.zeros(B, M, M, dtype=torch.int64, device=dev)
        self.track, self.age, self.origin, self.fate = i32(B, M), i32(B, M), i32(B, M), i32(B, M)
        self.step, self.path = f32(B, M), f32(B, M)
        self.track_map = i32(B, H, W)
        self.next_id = torch.ones(B, dtype=torch.int32, device=dev)
        # the previous frame: what the last push left
        self.prev_ids, self.prev_count = i32(B, H, W), i32(B)
        self.prev_sums = torch.zeros(B, M, SEG_SUMS, dtype=torch.int64, device=dev)
        self.prev_track, self.prev_age, self.prev_path = i32(B, M), i32(B, M), f32(B, M)
        first = grid == "first"
        self.flow_prev = f32(B, 2, H, W) if first else None                # pair k's forward and backward flow, kept for push k + 1
        self.flow_cur = f32(B, 2, H, W) if first else None
        self.mask_prev = torch.zeros(B, H, W, dtype=torch.uint8, device=dev) if first else None
        self.mask_cur = torch.zeros(B, H, W, dtype=torch.uint8, device=dev) if first else None

    def _buffers(self):
        names = ("votes", "track", "age", "origin", "fate", "step", "path", "track_map", "next_id", "prev_ids", "prev_count", "prev_sums",
                 "prev_track", "prev_age", "prev_path", "flow_prev", "flow_cur", "mask_prev", "mask_cur")
        return {getattr(self, n).data_ptr(): n for n in names if getattr(self, n) is not None}

    def reset(self):
        """Empties the state on the device (no track, next_id = 1): the next push makes every object new, through the same
        launches."""
        with _on(self.device):
            for t in (self.prev_ids, self.prev_count, self.prev_sums, self.prev_track, self.prev_age, self.prev_path, self.flow_prev,
                      self.flow_cur, self.mask_prev, self.mask_cur):
                if t is not None:
                    t.zero_()
            self.next_id.fill_(1)

    def _check(self, what, flow_on_prev, flow_on_cur, mask_prev, mask_cur):
        B, H, W, dev = self.B, self.H, self.W, self.device
        if flow_on_prev is None and flow_on_cur is None:
            raise PfError(f"{what}: at least one flow is required")
        mine = self._buffers()
        for name, t, shape, dt in (("flow_on_prev", flow_on_prev, (B, 2, H, W), torch.float32),
                                   ("flow_on_cur", flow_on_cur, (B, 2, H, W), torch.float32),
                                   ("mask_prev", mask_prev, (B, H, W), torch.uint8), ("mask_cur", mask_cur, (B, H, W), torch.uint8)):
            if t is None:
                continue
            _fit(t, shape, f"{what}: {name}", dev, dt)
            if t.data_ptr() in mine:
                raise PfError(f"{what}: {name} aliases {mine[t.data_ptr()]}")

    def _launch(self, flow_on_prev, flow_on_cur, mask_prev, mask_cur):
        o, lib = self.objects, self.lib
        n_dir = (flow_on_prev is not None) + (flow_on_cur is not None)
        with _on(self.device):
            lib.trk_begin(self.votes)
            lib.trk_vote(self.prev_ids, o.ids, flow_on_prev, flow_on_cur, mask_prev, mask_cur, o.rows, self.votes)
            lib.trk_match(self.votes, o.count, o.sums, self.prev_count, self.prev_sums, self.prev_track, self.prev_age, self.prev_path,
                          self.next_id, self.track, self.age, self.origin, self.fate, self.step, self.path, n_dir, self.min_overlap)
            lib.trk_paint(o.ids, self.track, self.track_map, self.prev_ids)
        return self.track, self.age, self.track_map

    def link(self, flow_on_prev, flow_on_cur, mask_prev=None, mask_cur=None):
        """The launches alone: links the objects the last push (or link) saw with ``objects``' current ones.  flow_on_prev fp32
        [B,2,H,W] lives on the previous objects' grid and points into the current frame, flow_on_cur on the current objects' grid
        and points back; either may be None.  mask_prev, mask_cur uint8 [B,H,W] or None: pixels with a non-zero byte do not vote.
        -> (track, age, track_map)."""
        self._check("ObjectTracker.link", flow_on_prev, flow_on_cur, mask_prev, mask_cur)
        return self._launch(flow_on_prev, flow_on_cur, mask_prev, mask_cur)

    def push(self, r):
        """(track int32 [B,M], age int32 [B,M], track_map int32 [B,H,W]) after ``objects.update*`` on the same pair r (a
        ``BidirectionalFlow``: forward, backward fp32 [B,2,H,W]; occ_forward, occ_backward uint8 [B,H,W] or None)."""
        try:
            fw, bw, ofw, obw = r.forward, r.backward, r.occ_forward, r.occ_backward
        except AttributeError:
            raise PfError(f"ObjectTracker.push: expected a BidirectionalFlow, got {type(r).__name__}") from None
        if fw is None or bw is None:
            raise PfError("ObjectTracker.push: the pair needs both flows")
        self._check("ObjectTracker.push", fw, bw, ofw, obw)
        if self.grid == "second":
            return self._launch(fw, bw, ofw, obw)
        out = self._launch(self.flow_prev, self.flow_cur, self.mask_prev, self.mask_cur)
        with _on(self.device):                                             # this pair links the next push
            self.flow_prev.copy_(fw)
            self.flow_cur.copy_(bw)
            if ofw is None:
                self.mask_prev.zero_()
            else:
                self.mask_prev.copy_(ofw)
            if obw is None:
                self.mask_cur.zero_()
            else:
                self.mask_cur.copy_(obw)
        return out
