"""Panoramic video inference: flow between consecutive frames with each frame encoded once, optionally warm-started.

    stream = FlowStream(model, iters=12, warm_start=True)
    for frame in frames:               # [B,3,H,W] on the device, 0..255 (B videos in lockstep)
        flow = stream(frame)           # None for the first frame, else flow(prev -> frame) [B,2,H,W] (branch A, as test_mode)
    stream.flow_low                    # [B,2,H/8,W/8]: coords1_A - coords0 of the last pair
    flows = run_sequence(model, frames, iters=12, warm_start=False)     # T frames -> T-1 flows

A pair (t-1, t) of ``model(f_prev, f_t, test_mode=True)`` runs the input stage and fnet on both frames.  The stream keeps what
the next pair needs of a frame -- its prepared view-A / view-B images (cnet's input of the next pair) and fnet's features of
both views (fp32 rows: the warps and alternate_corr's level 0; the bf16 hi|lo twins fnet's last convolution writes: the corr
build) -- so a step runs the input stage on ONE frame (pf_prepare_frame) and fnet on its 2B images only.  cnet, the corr build
(or the pooled features), the iterations and the upsampling are the per-pair forward's, on the same ``Engine``.

warm_start: ``init_flow`` of pair t is ``forward_interpolate(flow_low of pair t-1, wrap=True)`` (RAFT's sequence warm start,
evaluate.py:25-44 of the reference, with ERP wrapping), computed on the device inside the step (pf_forward_interpolate); view B
gets it through flo_rotate as in ``Engine.init_coords``.  The first pair after a (re)start runs cold.

Graph replay: one HIP graph per (B, H, W, device, precision, alternate_corr, iters, warm); the new frame's input stage runs in
front of the replay and the convex upsampling behind it (as ``PriOr_RAFT._run_graph``); the move of the new frame into the
cached slots (three device copies) is the graph's last work.  A step that captures runs eagerly first: the capture itself
executes nothing.

What is not reused: cnet runs on every pair (its input is the pair's first frame, which the previous pair used as its second),
the corr volumes / pooled features are rebuilt (they pair two frames), and fnet's outputs are copied once into the pair's slots.

Both directions:

    stream = FlowStream(model, iters=12, bidirectional=True, occlusion="sphere")      # or "plane", or None
    r = stream(frame)      # None for the first frame, else BidirectionalFlow(forward, backward, occ_forward, occ_backward,
                           # residual_forward, residual_backward): flow(prev -> frame), flow(frame -> prev), and
                           # forward_backward_check of the two
    stream.flow_low, stream.flow_low_backward

The pairs (prev, frame) and (frame, prev) are independent samples and run as ONE batch of 2B through the same ``Engine``
(``_BiState``: a frame's slot is its index modulo 2; sample block j is the pair whose first image is the frame in slot j).  The
backward pair's first image is the new frame, so cnet of the new frame, computed for it now, is the forward pair's context at the
next step: per step one input stage, fnet on 2B images and cnet on 2B images, the rest on the 2B workspace.  Warm start of the
backward pair: ``-forward_interpolate(-flow_low_backward of the previous pair, wrap=True)``.  One graph per (iters, warm, parity).
"""
from __future__ import annotations

import os
from collections import namedtuple
from typing import Dict, Iterable, List, Optional

import torch

from . import _lib
from ._lib import EPI_LINEAR, EPI_TANH_RELU, PREC_BF16X3, PfError
from .engine import Engine, Workspace


class _StreamState:
    """The device buffers of one (B, H, W, device, mode) stream: its own Workspace (a plain model(...) call never touches it),
    fnet's output of the new frame, the flows of the warm start and the scratch of pf_forward_interpolate."""

    def __init__(self, lib: _lib.PfLib, B: int, H: int, W: int, device, f16: bool, alt: bool):
        self.ws = ws = Workspace(lib, B, H, W, device, f16=f16, alt_corr=alt)
        rows = B * ws.N
        self.rows = rows
        # the prepared images: the new frame in the first half of the (otherwise unused) fnet batch, the cached frame in cnet's
        self.img_new = ws.img_f[:2 * B]
        self.img_prev = ws.img_c
        self.fn = torch.zeros(2 * rows, 256, dtype=torch.float32, device=device)        # fnet(new frame): [view A | view B]
        self.fn_split = None if ws.f_split is None else torch.zeros(2 * rows, 8, 2, 32, dtype=torch.bfloat16, device=device)
        # the pair's feature slots (ws.f_all = [f1A | f2A | f1B | f2B]): [view][first / second frame]
        self.f4 = ws.f_all.view(2, 2, rows, 256)
        self.s4 = None if ws.f_split is None else ws.f_split.view(2, 2, rows, 8, 2, 32)
        self.flow_low = torch.zeros(B, 2, ws.H8, ws.W8, dtype=torch.float32, device=device)
        self.init = torch.zeros_like(self.flow_low)
        self.scratch = torch.zeros(lib.forward_interpolate_scratch_bytes(B, ws.H8, ws.W8) // 4, dtype=torch.int32, device=device)
        self.have_frame = False         # a frame is cached (the next call returns a flow)
        self.have_flow = False          # flow_low holds a pair's result (the next pair may warm-start)
        self.graphs: Dict[tuple, torch.cuda.CUDAGraph] = {}
        self.keep = []                  # the encoders' activation sets the graphs point into (kept alive with them)


BidirectionalFlow = namedtuple("BidirectionalFlow", "forward backward occ_forward occ_backward residual_forward residual_backward")


def forward_backward_check(flow_fw: torch.Tensor, flow_bw: torch.Tensor, metric: str = "sphere", alpha: float = 0.01,
                           beta: float = 0.5, out=None):
    """Forward-backward consistency of two opposite panoramic flows [B,2,H,W] (flow_fw on the first frame's grid, flow_bw on
    the second's), both directions in one launch (pf_fb_check): -> (occ_fw, occ_bw, res_fw, res_bw), occ_* uint8 [B,H,W] with
    1 where the round trip p -> p + f -> p + f + g(p + f) fails, res_* that round trip in pixels (u across the seam).
    metric "sphere": the test compares great-circle lengths, beta in squared pixels at the equator; "plane": pixels.
    out: the four tensors to write into.  Capturable; CPU tensors are refused."""
    if not (flow_fw.is_cuda and flow_bw.is_cuda):
        raise PfError("forward_backward_check needs flows on a cuda/ROCm device; there is no CPU fallback")
    lib = _lib.load()
    with torch.no_grad(), torch.cuda.device(flow_fw.device):
        fw, bw = flow_fw.float().contiguous(), flow_bw.float().contiguous()
        if fw.dim() != 4 or fw.shape[1] != 2 or bw.shape != fw.shape:
            raise PfError(f"forward_backward_check: flows {tuple(fw.shape)} / {tuple(bw.shape)}, expected two [B,2,H,W] tensors")
        B, _, H, W = fw.shape
        if out is None:
            out = (torch.empty(B, H, W, dtype=torch.uint8, device=fw.device), torch.empty(B, H, W, dtype=torch.uint8, device=fw.device),
                   torch.empty_like(fw), torch.empty_like(fw))
        lib.fb_check(fw, bw, *out, metric=metric, alpha=alpha, beta=beta)
    return tuple(out)


class _BiState:
    """The device buffers of one bidirectional (B, H, W, device, mode) stream.  Its Workspace has batch 2B: sample block j
    (B samples) is the pair whose FIRST image is the frame in slot j, a frame's slot being its index modulo 2.  So the
    workspace's first images (and cnet's outputs) are [slot 0 | slot 1], its second images [slot 1 | slot 0]; a new frame
    overwrites one slot, nothing moves at the end of a step, and the block of the new frame's slot is the backward pair."""

    def __init__(self, lib: _lib.PfLib, B: int, H: int, W: int, device, f16: bool, alt: bool, twins: bool):
        self.B = B
        self.ws = ws = Workspace(lib, 2 * B, H, W, device, f16=f16, alt_corr=alt)
        self.rows = rows = B * ws.N              # rows of one view of one frame
        self.twins = twins                       # cnet writes split twins of its outputs (bf16x3 pre-split mode)
        self.img_new = ws.img_f[:2 * B]          # the new frame's prepared images [view A | view B]
        self.img_slot = ws.img_c.view(2, 2 * B, 3, H, W)       # the prepared images of the frame in each slot
        self.fn = torch.zeros(2 * rows, 256, dtype=torch.float32, device=device)
        self.fn_split = None if ws.f_split is None else torch.zeros(2 * rows, 8, 2, 32, dtype=torch.bfloat16, device=device)
        # ws.f_all = [f1A | f2A | f1B | f2B], each [block 0 | block 1]: [view][first / second image][block]
        self.f5 = ws.f_all.view(2, 2, 2, rows, 256)
        self.s5 = None if ws.f_split is None else ws.f_split.view(2, 2, 2, rows, 8, 2, 32)
        # cnet's outputs of the frame in each slot ([view A | view B] rows); the workspace's copies are the iterations' state
        z = lambda c: [torch.zeros(2 * rows, c, dtype=torch.float32, device=device) for _ in range(2)]  # noqa: E731
        self.cn_net = z(128)
        self.cn_x = None if twins else z(256)
        self.cn_net_s = [torch.zeros(2 * rows, 4, 2, 32, dtype=torch.bfloat16, device=device) for _ in range(2)] if twins else None
        self.cn_x_s = [torch.zeros(2 * rows, 8, 2, 32, dtype=torch.bfloat16, device=device) for _ in range(2)] if twins else None
        self.flow_low = torch.zeros(2 * B, 2, ws.H8, ws.W8, dtype=torch.float32, device=device)     # per block
        self.init = torch.zeros_like(self.flow_low)
        self.fi_in = torch.zeros_like(self.flow_low)
        self.scratch = torch.zeros(lib.forward_interpolate_scratch_bytes(2 * B, ws.H8, ws.W8) // 4, dtype=torch.int32, device=device)
        self.t = 0                      # frames seen since the (re)start: the next frame goes to slot t % 2
        self.have_flow = False
        self.fw_block = 0               # the block that held the forward pair of the last step
        self.graphs: Dict[tuple, torch.cuda.CUDAGraph] = {}
        self.keep = []


class FlowStream:
    """Flow of consecutive frames of B panoramic videos in lockstep: each frame goes through the input stage and fnet once
    (module docstring).  ``use_graph`` None follows ``model.use_graph``.  Inference only: a model in ``train()`` mode with
    autograd on is refused (PfError).

    ``bidirectional``: every call after the first returns a ``BidirectionalFlow`` -- ``forward`` = flow(previous -> frame),
    ``backward`` = flow(frame -> previous), and with ``occlusion`` "sphere" | "plane" the forward-backward masks and round
    trips of ``forward_backward_check`` on those two flows (None otherwise).  Both directions run as one batch of 2B; cnet runs
    on the new frame only (module docstring, "Both directions")."""

    def __init__(self, model, iters: int = 12, warm_start: bool = True, use_graph: Optional[bool] = None,
                 bidirectional: bool = False, occlusion: Optional[str] = None):
        if occlusion not in (None, "sphere", "plane"):
            raise PfError(f"FlowStream: occlusion {occlusion!r}, expected 'sphere', 'plane' or None")
        if occlusion is not None and not bidirectional:
            raise PfError("FlowStream: occlusion masks need bidirectional=True (they compare the two directions)")
        self.model = model
        self.iters = int(iters)
        self.warm_start = bool(warm_start)
        self.use_graph = use_graph
        self.bidirectional = bool(bidirectional)
        self.occlusion = occlusion
        self._st = None                 # _StreamState, or _BiState of a bidirectional stream
        self._key = None
        self._sig = None

    # ---- public ---------------------------------------------------------------------------------------------------------
    def reset(self) -> None:
        """Forget the cached frame and the last flow (the buffers and graphs stay): the next call returns None."""
        if self._st is not None:
            self._st.have_flow = False
            if self.bidirectional:
                self._st.t = 0
            else:
                self._st.have_frame = False

    @property
    def flow_low(self) -> Optional[torch.Tensor]:
        """coords1_A - coords0 of the last (forward) pair, [B,2,H/8,W/8] (a copy), or None before the first pair."""
        if self._st is None or not self._st.have_flow:
            return None
        if self.bidirectional:
            return self._block(self._st.flow_low, self._st.fw_block).clone()
        return self._st.flow_low.clone()

    @property
    def flow_low_backward(self) -> Optional[torch.Tensor]:
        """The same of the last backward pair (frame -> previous frame); bidirectional streams only."""
        if not self.bidirectional or self._st is None or not self._st.have_flow:
            return None
        return self._block(self._st.flow_low, 1 - self._st.fw_block).clone()

    def _block(self, t: torch.Tensor, j: int) -> torch.Tensor:
        """Sample block j of a tensor over the 2B samples of a bidirectional workspace."""
        B = self._st.B
        return t[j * B:(j + 1) * B]

    def __call__(self, frame: torch.Tensor) -> Optional[torch.Tensor]:
        m = self.model
        if not frame.is_cuda:
            raise PfError("FlowStream needs frames on a cuda/ROCm device; there is no CPU fallback")
        if torch.is_grad_enabled() and m.training and any(p.requires_grad for p in m.parameters()):
            raise PfError("FlowStream is inference-only: call model.eval() or run it under torch.no_grad()")
        if frame.dim() != 4 or frame.shape[1] != 3:
            raise PfError(f"FlowStream: frame {tuple(frame.shape)}, expected [B,3,H,W]")
        B, _, H, W = frame.shape
        device = frame.device
        with torch.no_grad(), torch.cuda.device(device):
            frame = frame.float().contiguous()
            lib = m._lib()
            P = m._weights()
            plans = m._encoder_plans()
            key = (B, H, W, str(device), P["precision"], m._alt_corr())
            if self.bidirectional:
                return self._call_bidirectional(frame, key, lib, P, plans)
            if key != self._key:            # new shape, device or mode: a fresh stream
                self._st = _StreamState(lib, B, H, W, device, P["precision"] == _lib.PREC_F16, m._alt_corr())
                self._key = key
                self._sig = None
            st = self._st
            sig = (P, plans)                # (held, so a rebuilt object can never reuse an old one's identity)
            if self._sig is None or sig[0] is not self._sig[0] or sig[1] is not self._sig[1]:
                # packed weights or encoder plans were rebuilt (an in-place edit, a precision switch): the graphs hold pointers to the
                # old ones, and the cached frame's features came from the old fnet
                st.graphs.clear()
                st.keep = []
                if st.have_frame and self._sig is not None:
                    self._encode_cached(st, plans[1], P)
                self._sig = sig
            lib.prepare_frame(frame, st.ws.g_a2b, st.img_new)
            if not st.have_frame:
                self._prime(st, plans[1], P)
                return None
            warm = self.warm_start and st.have_flow
            use_graph = (m.use_graph if self.use_graph is None else self.use_graph) and not m.training
            gkey = (self.iters, warm)
            graph = st.graphs.get(gkey) if use_graph else None
            if graph is not None:
                graph.replay()
            else:
                self._step(st, warm)
                if use_graph:
                    graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graph):
                        self._step(st, warm)
                    st.graphs[gkey] = graph
                    st.keep.append([p._bufs for p in plans])
            st.have_flow = True
            out = torch.empty(B, 2, H, W, dtype=torch.float32, device=device)
            Engine(lib, None).upsample(st.ws, "a", out)
            return out

    # ---- internals ------------------------------------------------------------------------------------------------------
    def _fsplit(self, st: _StreamState, fplan, P) -> dict:
        """fnet's last convolution writes the bf16 twins of its features as well when the corr build multiplies those."""
        ok = st.fn_split is not None and Engine.encoder_precision(P) == PREC_BF16X3 and fplan.precision == PREC_BF16X3
        return dict(outs=st.fn_split) if ok else {}

    def _encode_new(self, st: _StreamState, fplan, P, slot: int):
        """fnet on the new frame's 2B images, its rows copied into the pair's feature slots `slot` (0: first frame, 1: second)."""
        fs = self._fsplit(st, fplan, P)
        fplan.run(st.img_new, st.fn, EPI_LINEAR, **fs)
        st.f4[:, slot].copy_(st.fn.view(2, st.rows, 256))
        if fs:
            st.s4[:, slot].copy_(st.fn_split.view(2, st.rows, 8, 2, 32))
        return bool(fs)

    def _prime(self, st: _StreamState, fplan, P):
        """The first frame: encoded into the cached slots, its prepared images kept for cnet."""
        self._encode_new(st, fplan, P, 0)
        st.img_prev.copy_(st.img_new)
        st.have_frame = True
        st.have_flow = False

    def _encode_cached(self, st: _StreamState, fplan, P):
        """Re-encode the cached frame from its prepared images (its features came from weights that have changed since)."""
        st.img_new.copy_(st.img_prev)
        self._encode_new(st, fplan, P, 0)

    def _step(self, st: _StreamState, warm: bool):
        """One pair (cached frame -> new frame), up to and excluding the upsampling; the structure of PriOr_RAFT._encode + _run
        (test_mode) with fnet on the new frame only.  Ends by moving the new frame into the cached slots."""
        m = self.model
        lib, P = m._lib(), m._weights()
        cplan, fplan = m._encoder_plans()
        ws = st.ws
        eng = Engine(lib, m._streams() if m.use_streams else None)
        ws.pre_ready = False
        f16 = ws.f16
        ctx = dict(outs=ws.net0_ab_s, auxs=ws.x_ab_s) if eng.presplit(P) and not f16 else dict(aux=ws.x_ab)

        def context():
            cplan.run(st.img_prev, ws.net0_ab, EPI_TANH_RELU, **ctx)
            if f16:
                lib.split_f16(ws.net0_ab, ws.net0_ab_s)
                lib.split_f16(ws.x_ab[:, :128], ws.x_ab_s)
            eng.hoist_context(ws, P)

        def features():
            ws.f_split_ready = self._encode_new(st, fplan, P, 1)
            eng.build_pyramids(ws, Engine.encoder_precision(P))

        def coords():
            if warm:
                lib.forward_interpolate(st.flow_low, st.init, st.scratch, wrap=True)
            eng.init_coords(ws, st.init if warm else None)

        if m.use_streams and int(os.environ.get("PRIORFLOW_FORKS", "15")) & 1:
            cur = torch.cuda.current_stream()
            s1, s2 = m._streams()[:2]
            ev = torch.cuda.Event()
            ev.record(cur)
            context()
            s1.wait_event(ev)
            with torch.cuda.stream(s1):
                features()
            s2.wait_event(ev)
            with torch.cuda.stream(s2):
                coords()
            cur.wait_stream(s1)
            cur.wait_stream(s2)
        else:
            coords()
            context()
            features()
        cur_state = 0
        for it in range(self.iters):
            last = it == self.iters - 1
            cur_state = eng.iteration(ws, P, cur_state, need_b=not last, mask_a=last, mask_b=False, defer_b_join=not last)
        torch.sub(ws.c1a, ws.coords0, out=st.flow_low)
        # the new frame becomes the cached one
        st.f4[:, 0].copy_(st.f4[:, 1])
        if st.s4 is not None and ws.f_split_ready:
            st.s4[:, 0].copy_(st.s4[:, 1])
        st.img_prev.copy_(st.img_new)


    # ---- both directions (module docstring) ------------------------------------------------------------------------------
    def _call_bidirectional(self, frame: torch.Tensor, key, lib, P, plans):
        """One call of a bidirectional stream, after the argument checks (inside no_grad and the frame's device)."""
        m = self.model
        B, _, H, W = frame.shape
        if key != self._key:
            twins = Engine(lib, None).presplit(P) and P["precision"] != _lib.PREC_F16
            self._st = _BiState(lib, B, H, W, frame.device, P["precision"] == _lib.PREC_F16, m._alt_corr(), twins)
            self._key = key
            self._sig = None
        st = self._st
        sig = (P, plans)
        if self._sig is None or sig[0] is not self._sig[0] or sig[1] is not self._sig[1]:
            # rebuilt weights or plans: the graphs point into the old ones, and the cached frame's features AND cnet outputs
            # came from the old encoders
            st.graphs.clear()
            st.keep = []
            if st.t > 0 and self._sig is not None:
                slot = (st.t - 1) % 2
                st.img_new.copy_(st.img_slot[slot])
                self._encode_frame(st, plans, P, slot)
            self._sig = sig
        lib.prepare_frame(frame, st.ws.g_a2b, st.img_new)
        slot = st.t % 2
        if st.t == 0:
            self._encode_frame(st, plans, P, slot)
            st.img_slot[slot].copy_(st.img_new)
            st.t, st.have_flow = 1, False
            return None
        warm = self.warm_start and st.have_flow
        use_graph = (m.use_graph if self.use_graph is None else self.use_graph) and not m.training
        gkey = (self.iters, warm, slot)     # (the stream's state is bidirectional already; the check runs behind the graph)
        graph = st.graphs.get(gkey) if use_graph else None
        if graph is not None:
            graph.replay()
        else:
            self._step_bidirectional(st, warm, slot)
            if use_graph:
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    self._step_bidirectional(st, warm, slot)
                st.graphs[gkey] = graph
                st.keep.append([p._bufs for p in plans])
        st.t += 1
        st.have_flow = True
        st.fw_block = 1 - slot              # the new frame is the FIRST image of its own block: that pair runs backwards
        out = torch.empty(2 * B, 2, H, W, dtype=torch.float32, device=frame.device)
        Engine(lib, None).upsample(st.ws, "a", out)
        fw, bw = self._block(out, st.fw_block), self._block(out, slot)
        if self.occlusion is None:
            return BidirectionalFlow(fw, bw, None, None, None, None)
        return BidirectionalFlow(fw, bw, *forward_backward_check(fw, bw, metric=self.occlusion))

    def _encode_features(self, st: _BiState, fplan, P, slot: int) -> bool:
        """fnet on the 2B images in st.img_new, stored as the frame of `slot`: the first image of block `slot` and the second
        image of the other block."""
        fs = self._fsplit(st, fplan, P)
        fplan.run(st.img_new, st.fn, EPI_LINEAR, **fs)
        v = st.fn.view(2, st.rows, 256)
        st.f5[:, 0, slot].copy_(v)
        st.f5[:, 1, 1 - slot].copy_(v)
        if fs:
            v = st.fn_split.view(2, st.rows, 8, 2, 32)
            st.s5[:, 0, slot].copy_(v)
            st.s5[:, 1, 1 - slot].copy_(v)
        return bool(fs)

    def _encode_context(self, st: _BiState, cplan, slot: int):
        """cnet on the same 2B images, into the slot's cache (the forward pair of the NEXT step reads it from there)."""
        if st.twins:
            cplan.run(st.img_new, st.cn_net[slot], EPI_TANH_RELU, outs=st.cn_net_s[slot], auxs=st.cn_x_s[slot])
        else:
            cplan.run(st.img_new, st.cn_net[slot], EPI_TANH_RELU, aux=st.cn_x[slot])

    def _encode_frame(self, st: _BiState, plans, P, slot: int):
        self._encode_context(st, plans[0], slot)
        self._encode_features(st, plans[1], P, slot)

    def _context_in(self, st: _BiState, lib):
        """cnet's cached outputs of both slots -> the workspace (net is the iterations' state: they overwrite it; of the x
        buffer the context half only)."""
        ws, r = st.ws, st.rows
        for j in range(2):
            ws.net0_ab.view(2, 2, r, 128)[:, j].copy_(st.cn_net[j].view(2, r, 128))
            if st.twins:
                ws.net0_ab_s.view(2, 2, r, 4, 2, 32)[:, j].copy_(st.cn_net_s[j].view(2, r, 4, 2, 32))
                ws.x_ab_s.view(2, 2, r, 8, 2, 32)[:, j, :, :4].copy_(st.cn_x_s[j].view(2, r, 8, 2, 32)[:, :, :4])
            else:
                ws.x_ab.view(2, 2, r, 256)[:, j, :, :128].copy_(st.cn_x[j].view(2, r, 256)[:, :, :128])
        if ws.f16:
            lib.split_f16(ws.net0_ab, ws.net0_ab_s)
            lib.split_f16(ws.x_ab[:, :128], ws.x_ab_s)

    def _step_bidirectional(self, st: _BiState, warm: bool, slot: int):
        """Both pairs of (cached frame, new frame) as one batch of 2B, up to and excluding the upsampling: the new frame (in
        st.img_new) goes through fnet and cnet and into `slot`; block `slot` is then the backward pair, the other the forward."""
        m = self.model
        lib, P = m._lib(), m._weights()
        plans = m._encoder_plans()
        ws, B = st.ws, st.B
        eng = Engine(lib, m._streams() if m.use_streams else None)
        ws.pre_ready = False

        def context():
            self._encode_context(st, plans[0], slot)
            self._context_in(st, lib)
            eng.hoist_context(ws, P)

        def features():
            ws.f_split_ready = self._encode_features(st, plans[1], P, slot)
            eng.build_pyramids(ws, Engine.encoder_precision(P))

        def coords():
            if warm:
                # the last step's forward pair sat in block `slot`, its backward pair in the other one; now the other way round.
                # forward: forward_interpolate(flow_low); backward: -forward_interpolate(-flow_low_backward) (constant velocity)
                low, src, init = (t.view(2, B, 2, ws.H8, ws.W8) for t in (st.flow_low, st.fi_in, st.init))
                src[1 - slot].copy_(low[slot])
                torch.neg(low[1 - slot], out=src[slot])
                lib.forward_interpolate(st.fi_in, st.init, st.scratch, wrap=True)
                init[slot].neg_()
            eng.init_coords(ws, st.init if warm else None)

        if m.use_streams and int(os.environ.get("PRIORFLOW_FORKS", "15")) & 1:
            cur = torch.cuda.current_stream()
            s1, s2 = m._streams()[:2]
            ev = torch.cuda.Event()
            ev.record(cur)
            context()
            s1.wait_event(ev)
            with torch.cuda.stream(s1):
                features()
            s2.wait_event(ev)
            with torch.cuda.stream(s2):
                coords()
            cur.wait_stream(s1)
            cur.wait_stream(s2)
        else:
            coords()
            context()
            features()
        cur_state = 0
        for it in range(self.iters):
            last = it == self.iters - 1
            cur_state = eng.iteration(ws, P, cur_state, need_b=not last, mask_a=last, mask_b=False, defer_b_join=not last)
        torch.sub(ws.c1a, ws.coords0, out=st.flow_low)
        st.img_slot[slot].copy_(st.img_new)


def run_sequence(model, frames: Iterable[torch.Tensor], iters: int = 12, warm_start: bool = False,
                 use_graph: Optional[bool] = None, bidirectional: bool = False, occlusion: Optional[str] = None) -> List:
    """T frames ([B,3,H,W] each, or one [T,B,3,H,W] tensor) -> the T-1 flows of consecutive pairs (bidirectional: the T-1
    ``BidirectionalFlow`` tuples)."""
    stream = FlowStream(model, iters=iters, warm_start=warm_start, use_graph=use_graph, bidirectional=bidirectional,
                        occlusion=occlusion)
    flows = []
    for frame in frames:
        flow = stream(frame)
        if flow is not None:
            flows.append(flow)
    return flows
