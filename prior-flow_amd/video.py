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
"""
from __future__ import annotations

import os
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


class FlowStream:
    """Flow of consecutive frames of B panoramic videos in lockstep: each frame goes through the input stage and fnet once
    (module docstring).  ``use_graph`` None follows ``model.use_graph``.  Inference only: a model in ``train()`` mode with
    autograd on is refused (PfError)."""

    def __init__(self, model, iters: int = 12, warm_start: bool = True, use_graph: Optional[bool] = None):
        self.model = model
        self.iters = int(iters)
        self.warm_start = bool(warm_start)
        self.use_graph = use_graph
        self._st: Optional[_StreamState] = None
        self._key = None
        self._sig = None

    # ---- public ---------------------------------------------------------------------------------------------------------
    def reset(self) -> None:
        """Forget the cached frame and the last flow (the buffers and graphs stay): the next call returns None."""
        if self._st is not None:
            self._st.have_frame = self._st.have_flow = False

    @property
    def flow_low(self) -> Optional[torch.Tensor]:
        """coords1_A - coords0 of the last pair, [B,2,H/8,W/8] (a copy), or None before the first pair."""
        if self._st is None or not self._st.have_flow:
            return None
        return self._st.flow_low.clone()

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


def run_sequence(model, frames: Iterable[torch.Tensor], iters: int = 12, warm_start: bool = False,
                 use_graph: Optional[bool] = None) -> List[torch.Tensor]:
    """T frames ([B,3,H,W] each, or one [T,B,3,H,W] tensor) -> the T-1 flows of consecutive pairs."""
    stream = FlowStream(model, iters=iters, warm_start=warm_start, use_graph=use_graph)
    flows = []
    for frame in frames:
        flow = stream(frame)
        if flow is not None:
            flows.append(flow)
    return flows
