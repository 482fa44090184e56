"""The training loop's backward (prior_flow_amd/train_loop.py: LoopFn) against float64 AT ITS SAVED STATE -- helper of
test_train_loop_reference.py (host) and test_hip_train_loop.py (GPU); not a conftest, no test functions.

WHAT IS COMPARED.  LoopFn.backward is the vector-Jacobian product of the refinement loop at the forward state the forward
saved.  Two correct float32 / float64 implementations of the loop differ by 1e-2 in their gradients, not by rounding: a
pre-activation near zero flips a ReLU mask, a derived sample coordinate crosses the zero-padded wrap seam of the cyclic
sampler.  So the float64 reference here is PINNED to the state of the run under test (`State`):

  * every iteration starts from the saved coordinates c[i] (detached in the model anyway), flow_B seen from A is the saved one;
  * every ReLU is x * (saved output > 0);
  * the sampled values (both correlation lookups, both warped group correlations) are the saved ones through a straight-
    through pin, ref + (saved - ref).detach(): the values are those of the run under test, the derivative -- towards the
    pyramids and towards f1 / f2 -- is the reference's.

`loop_body` is the loop body of core/prior_raft.py:170-211 with core/update.py's blocks written out (the samplers, lookups and
the convex upsampling are the oracle's functions); it runs in float32 or float64 on any device, free (its own state, which it
records: the host test's "kernel") or pinned.  torch.autograd.backward on the same seeds gives the 6 leaf gradients, the 8
pyramid-level gradients and every update-block weight / bias gradient.

WHERE THE TOLERANCE COMES FROM (`check`).  Not a chosen number and not measured on the kernels: the ROUNDING MODEL is the same
pinned graph in float32 in which every convolution with more than 2 input channels rounds both operands to bf16 hi + bf16 lo
(what pf_split_bf16 keeps) in the forward, the data-gradient and the weight-gradient pass (`conv_split`); the 2-channel 7x7
stems stay plain fp32, as pf_conv2d_small is.  For output tensor t, E_t = ||model_t - ref_t|| / ||ref_t||, and the run under
test must satisfy
        ||got_t - ref_t|| <= K_AGG * E_t * ||ref_t|| + 1e-7 * max_t ||ref_t||
with conv_launches.K_AGG = 8, the project's margin for a random walk of independent roundings whose summation order differs
from the one realisation the model gives.  The absolute term is applied ONLY to a tensor whose reference norm is itself below
it (a true gradient of zero): max_t ||ref_t|| is a large weight gradient's (5.8e3 at B=1, 17x27), and added to every bound the
term would be 290x the rounding part of d_f1 / d_f2 (norm 0.03) and 10-36x that of the pyramid levels and conv_conf1 --
1e-3 to 2e-2 of their norms, the old tolerance again.  Every other tensor is held to K_AGG * E_t of its norm, below 1e-3
(asserted on the CPU).

SEAM CAP (a condition, not a tolerance; pyramid gradients only).  A cross-lookup sample that lands on the seam is routed to
another handful of pyramid elements by the two precisions: one event moves one bilinear sample between two sets of at most 4
elements.  Up to SEAM_CAP = 16 elements per pyramid tensor (two events) are left out of the norm: those with the largest
|err|, and only if each exceeds 100x the rms error of the tensor's other elements.  The same rule is applied to the model's
error (it lowers E_t, never raises it).  No other tensor gets a cap.
"""
from __future__ import annotations

import contextlib
from dataclasses import dataclass
from typing import Dict, List, Optional

import torch
import torch.nn.functional as F

import golden_cases as gc
import priorflow_oracle as po
from conv_launches import K_AGG

SEAM_CAP = 16
SEAM_FACTOR = 100.0
ABS_TERM = 1e-7
LEAVES = ("net_a", "net_b", "inp_a", "inp_b", "f1a", "f2a")
PYR = tuple(f"pyr_{t}{i}" for t in "ab" for i in range(4))


@dataclass(frozen=True)
class Case:
    name: str
    B: int
    H8: int
    W8: int
    iters: int
    seed: int
    last_only: bool = False     # only the last prediction of each branch carries a gradient seed; the others get zeros


# The smallest shapes at which the loop still goes wrong (H8 >= 8: four pyramid levels).  EVEN: even tiles, a live batch index,
# three iterations reuse both ping-pong pairs of the backward's scratch.  RAGGED: ragged conv / wgrad tiles, floor-pooled
# pyramid (17 -> 8 -> 4 -> 2), odd width at the seam.  The seeds are ones for which the float32 / float64 reference pair stays
# within the seam cap (test_train_loop_reference.py asserts it).
EVEN = Case("B2_16x32_it3", 2, 16, 32, 3, 1)
RAGGED = Case("B1_17x27_it4", 1, 17, 27, 4, 1)
EVEN_LAST = Case("B2_16x32_it3_last_only", 2, 16, 32, 3, 1, True)
EVEN_B = Case("B2_16x32_it3_second_set", 2, 16, 32, 3, 2)       # the second seeded set of the graph-replay test
INIT_FLOW = 3.0            # |init_flow| <= 3 px at 1/8 resolution: lookups (radius 4 on four levels) cross the ERP seam


# ---------------------------------------------------------------------------------------------------------------------
# seeded inputs
# ---------------------------------------------------------------------------------------------------------------------
def make_inputs(case: Case) -> dict:
    """CPU fp32: the six leaves, two pyramids (four [B*N, Hi*Wi] row tensors each, of seeded features of their own), init_flow
    and the 2 * iters gradient seeds (uniform [-1, 1]; `last_only`: zeros but for the last prediction of each branch)."""
    B, H8, W8, it = case.B, case.H8, case.W8, case.iters
    gen = torch.Generator().manual_seed(case.seed)
    r = lambda *s: torch.rand(*s, generator=gen, dtype=torch.float32) * 2 - 1      # noqa: E731
    inp = dict(net_a=torch.tanh(r(B, 128, H8, W8)), net_b=torch.tanh(r(B, 128, H8, W8)), inp_a=torch.relu(r(B, 128, H8, W8)),
               inp_b=torch.relu(r(B, 128, H8, W8)), f1a=r(B, 256, H8, W8), f2a=r(B, 256, H8, W8))
    feats = [r(B, 256, H8, W8) for _ in range(4)]
    for t, (f1, f2) in (("a", feats[:2]), ("b", feats[2:])):
        for i, lv in enumerate(po.build_pyramid(po.corr_volume(f1, f2))):
            inp[f"pyr_{t}{i}"] = lv.reshape(B * H8 * W8, -1).contiguous()
    inp["init_flow"] = r(B, 2, H8, W8) * INIT_FLOW
    seeds = [r(B, 2, 8 * H8, 8 * W8) for _ in range(2 * it)]
    if case.last_only:
        seeds = [s if k in (it - 1, 2 * it - 1) else torch.zeros_like(s) for k, s in enumerate(seeds)]
    inp["seeds"] = seeds
    return inp


_WEIGHTS: Dict[str, torch.Tensor] = {}


def update_weights() -> Dict[str, torch.Tensor]:
    """CPU fp32 parameters of the two update blocks (det_state_dict, the weights the GPU tests load into PriOr_RAFT)."""
    if not _WEIGHTS:
        from prior_flow_amd.modules import state_dict_shapes
        for k, v in gc.det_state_dict(state_dict_shapes()).items():
            if k.startswith(("ODDC.", "update_block.")) and v.dtype.is_floating_point:
                _WEIGHTS[k] = v
    return _WEIGHTS


def grids(case: Case, device, dtype) -> Dict[str, torch.Tensor]:
    """The oracle's 1/8 sample grids (computed in fp32 as the reference does), cast."""
    g = po.grids_for(8 * case.H8, 8 * case.W8)
    return {k: v.to(device=device, dtype=dtype) for k, v in g.items() if k.endswith("_8")}


# ---------------------------------------------------------------------------------------------------------------------
# convolutions
# ---------------------------------------------------------------------------------------------------------------------
def conv_taps(x, w, b, pad):
    """F.conv2d(x, w, b, padding=pad), stride 1, as one matmul per tap in x's dtype on x's device (conv_launches.conv_fp64's
    form: no library convolution takes part, so float64 on the GPU is float64)."""
    co, ci, kh, kw = w.shape
    B, _, H, W = x.shape
    xp = F.pad(x.permute(0, 2, 3, 1), (0, 0, pad[1], pad[1], pad[0], pad[0]))
    wt = w.permute(2, 3, 1, 0)
    y = None
    for ky in range(kh):
        for kx in range(kw):
            t = xp[:, ky:ky + H, kx:kx + W, :].reshape(-1, ci) @ wt[ky, kx]
            y = t if y is None else y + t
    if b is not None:
        y = y + b
    return y.view(B, H, W, co).permute(0, 3, 1, 2).contiguous()


def split_round(x):
    """bf16 hi + bf16 lo of an fp32 tensor: the 16 significant bits pf_split_bf16 keeps."""
    hi = x.bfloat16().float()
    lo = (x - hi).bfloat16().float()
    return hi + lo


class _ConvSplit(torch.autograd.Function):
    """The rounding model of one bf16x3 convolution: both operands rounded to hi + lo in the forward, in the data gradient
    (conv2d_input of the rounded weights and output gradient) and in the weight gradient (conv2d_weight of the rounded input
    and output gradient); fp32 accumulation; the bias and its gradient in fp32."""

    @staticmethod
    def forward(ctx, x, w, b, pad):
        ctx.save_for_backward(x, w)
        ctx.pad = pad
        return conv_taps(split_round(x), split_round(w), b, pad)

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        gr = split_round(gy)
        dx = dw = None
        with torch.enable_grad():
            if ctx.needs_input_grad[0]:
                xd = x.detach().requires_grad_(True)
                dx, = torch.autograd.grad(conv_taps(xd, split_round(w).detach(), None, ctx.pad), xd, gr)
            if ctx.needs_input_grad[1]:
                wd = w.detach().requires_grad_(True)
                dw, = torch.autograd.grad(conv_taps(split_round(x).detach(), wd, None, ctx.pad), wd, gr)
        return dx, dw, gy.sum((0, 2, 3)), None


def conv_plain(x, w, b, pad):
    return conv_taps(x, w, b, pad)


def conv_split(x, w, b, pad):
    """The rounding model's convolution: bf16 hi + lo operands where the product runs pf_conv2d (more than 2 input
    channels), plain fp32 where it runs pf_conv2d_small (the 2-channel 7x7 stems)."""
    if x.dtype == torch.float32 and x.shape[1] > 2:
        return _ConvSplit.apply(x, w, b, pad)
    return conv_taps(x, w, b, pad)


# ---------------------------------------------------------------------------------------------------------------------
# saved state
# ---------------------------------------------------------------------------------------------------------------------
RELUS_A = ("a.c1", "a.cor", "a.t_a", "a.flo_a", "a.t_ba", "a.flo_b", "a.cf1", "a.conf", "a.out", "a.fh", "a.mh")
RELUS_B = ("b.c1", "b.cor", "b.t", "b.flo", "b.out", "b.fh", "b.mh")
VALUES = ("c_a", "c_b", "corr_a", "corr_b", "flow_ba", "flaw_a", "flaw_ba")
State = List[Dict[str, torch.Tensor]]        # per iteration: VALUES and the outputs of RELUS_A / RELUS_B, NCHW


def state_from_buffers(bufs, case: Case) -> State:
    """Copies what the reference is pinned to out of model._loop_bufs (train_loop.LoopBuffers) after a forward."""
    B, H8, W8 = case.B, case.H8, case.W8
    A, Bb = bufs.a, bufs.b
    img = lambda rows: rows.view(B, H8, W8, -1).permute(0, 3, 1, 2).clone()        # noqa: E731
    st = []
    for i in range(case.iters):
        cat_a, cat_b = A["cat"][i], Bb["cat"][i]
        s = {"c_a": A["c"][i].clone(), "c_b": Bb["c"][i].clone(), "corr_a": img(A["corr"][i]), "corr_b": img(Bb["corr"][i]),
             "flow_ba": img(A["flow4"][i][:, 2:4]), "flaw_a": img(A["conf_in"][i][:, :4]), "flaw_ba": img(A["conf_in"][i][:, 4:8]),
             "a.c1": img(A["c1"][i]), "a.cor": img(cat_a[:, :128]), "a.flo_a": img(cat_a[:, 128:192]),
             "a.flo_b": img(cat_a[:, 192:256]), "a.conf": img(cat_a[:, 256:272]), "a.out": img(A["x"][i][:, 128:252]),
             "a.fh": img(A["fh"][i]), "a.mh": img(A["mh"][i]), "a.t_a": img(A["t_a"][i]), "a.t_ba": img(A["t_ba"][i]),
             "a.cf1": img(A["cf1"][i]),
             "b.c1": img(Bb["c1"][i]), "b.cor": img(cat_b[:, :192]), "b.flo": img(cat_b[:, 192:256]),
             "b.out": img(Bb["x"][i][:, 128:254]), "b.fh": img(Bb["fh"][i]), "b.mh": img(Bb["mh"][i]), "b.t": img(Bb["t"][i])}
        st.append(s)
    return st


# ---------------------------------------------------------------------------------------------------------------------
# seeded faults of the backward (host test): none of them changes a forward value
# ---------------------------------------------------------------------------------------------------------------------
FAULTS = ("flaw_ba_detached", "warp2_reads_conf_0_4", "mask_quarter_missing", "b_out_124_125_zero", "d_inp_last_only",
          "cross_detached", "hidden_not_handed_on", "stale_relu_mask", "d_c1_tile_zero")


class _GradOfFirst(torch.autograd.Function):
    """(a, b) -> (a, b); b's gradient is replaced by a's (the second warp backward reading the first one's columns)."""

    @staticmethod
    def forward(ctx, a, b):
        return a.clone(), b.clone()

    @staticmethod
    def backward(ctx, ga, gb):
        return ga, ga


class _ScaleGrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, s):
        ctx.s = s
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        return g * ctx.s, None


class _ReluStaleMask(torch.autograd.Function):
    """relu(x) whose backward multiplies by ANOTHER iteration's mask: a stale buffer, what a missed wait looks like."""

    @staticmethod
    def forward(ctx, x, stale):
        ctx.save_for_backward(stale)
        return F.relu(x)

    @staticmethod
    def backward(ctx, g):
        stale, = ctx.saved_tensors
        return g * (stale > 0).to(g.dtype), None


def _zero_grad_of(t, sl):
    def hook(g):
        g = g.clone()
        g[sl] = 0
        return g
    t.register_hook(hook)


# ---------------------------------------------------------------------------------------------------------------------
# the loop body
# ---------------------------------------------------------------------------------------------------------------------
class _Run:
    """One evaluation of the loop: the convolution to use, the pins (None: free) and the record being written."""

    def __init__(self, p, conv, pins: Optional[State], fault: Optional[str]):
        self.p, self.conv, self.pins, self.fault = p, conv, pins, fault
        self.rec: State = []
        self.i = 0

    def cv(self, name, x, pad):
        return self.conv(x, self.p[name + ".weight"], self.p[name + ".bias"], pad)

    def relu(self, key, x):
        if self.pins is not None:
            return x * (self.pins[self.i][key] > 0).to(x.dtype)
        if self.fault == "stale_relu_mask" and key == "a.c1" and self.i == 1:
            y = _ReluStaleMask.apply(x, self.rec[0][key])
        else:
            y = F.relu(x)
        self.rec[self.i][key] = y.detach()
        if self.fault == "b_out_124_125_zero" and key == "b.out":
            _zero_grad_of(y, (slice(None), slice(124, 126)))
        if self.fault == "d_c1_tile_zero" and key == "a.c1" and self.i == 1:
            _zero_grad_of(y, (0, slice(None), slice(4, 8), slice(8, 24)))       # strictly inside the map
        return y

    def value(self, key, ref):
        """A sampled value: recorded when free, straight-through pinned otherwise."""
        if self.pins is None:
            self.rec[self.i][key] = ref.detach()
            return ref
        return ref + (self.pins[self.i][key].to(ref.dtype) - ref).detach()


def _gru(run: _Run, pre, h, x):
    """SepConvGRU (core/update.py:35-60): the (1x5) pass, then the (5x1) pass."""
    for tag, pad in (("1", (0, 2)), ("2", (2, 0))):
        hx = torch.cat([h, x], 1)
        z = torch.sigmoid(run.cv(pre + "convz" + tag, hx, pad))
        r = torch.sigmoid(run.cv(pre + "convr" + tag, hx, pad))
        q = torch.tanh(run.cv(pre + "convq" + tag, torch.cat([r * h, x], 1), pad))
        h = (1 - z) * h + z * q
    return h


def _heads(run: _Run, pre, t, net):
    """FlowHead and the mask head (core/update.py:6-14, :124-127, :133-135, :157)."""
    delta = run.cv(pre + "flow_head.conv2", run.relu(t + ".fh", run.cv(pre + "flow_head.conv1", net, (1, 1))), (1, 1))
    mh = run.relu(t + ".mh", run.cv(pre + "mask.0", net, (1, 1)))
    if run.fault == "mask_quarter_missing" and t == "a":
        mh = _ScaleGrad.apply(mh, 4.0)          # the data gradient without the 0.25; the weight gradient keeps it
    return 0.25 * run.cv(pre + "mask.2", mh, (0, 0)), delta


def _update_a(run: _Run, net, inp, flow_a, corr, flaw_a, flow_ba, flaw_ba):
    """BasicMultiUpdateBlock + BasicMultiMotionEncoder (core/update.py:139-159, :162-201)."""
    e = "ODDC.encoder."
    cor = run.relu("a.cor", run.cv(e + "convc2_A", run.relu("a.c1", run.cv(e + "convc1_A", corr, (0, 0))), (1, 1)))
    fa = run.relu("a.flo_a", run.cv(e + "convf2_A", run.relu("a.t_a", run.cv(e + "convf1_A", flow_a, (3, 3))), (1, 1)))
    fb = run.relu("a.flo_b", run.cv(e + "convf2_B", run.relu("a.t_ba", run.cv(e + "convf1_B", flow_ba, (3, 3))), (1, 1)))
    conf = run.relu("a.cf1", run.cv(e + "conv_conf1", torch.cat([flaw_a, flaw_ba], 1), (1, 1)))
    conf = run.relu("a.conf", run.cv(e + "conv_conf2", conf, (1, 1)))
    out = run.relu("a.out", run.cv(e + "conv_A", torch.cat([cor, fa, fb, conf], 1), (1, 1)))
    net = _gru(run, "ODDC.gru.", net, torch.cat([inp, out, flow_a, flow_ba], 1))
    mask, delta = _heads(run, "ODDC.", "a", net)
    return net, mask, delta


def _update_b(run: _Run, net, inp, corr, flow):
    """BasicUpdateBlock + BasicMotionEncoder (core/update.py:117-136, :81-99)."""
    e = "update_block.encoder."
    cor = run.relu("b.cor", run.cv(e + "convc2", run.relu("b.c1", run.cv(e + "convc1", corr, (0, 0))), (1, 1)))
    fl = run.relu("b.flo", run.cv(e + "convf2", run.relu("b.t", run.cv(e + "convf1", flow, (3, 3))), (1, 1)))
    out = run.relu("b.out", run.cv(e + "conv", torch.cat([cor, fl], 1), (1, 1)))
    net = _gru(run, "update_block.gru.", net, torch.cat([inp, out, flow], 1))
    mask, delta = _heads(run, "update_block.", "b", net)
    return net, mask, delta


def loop_body(run: _Run, L, pyr_a, pyr_b, g, c1a, c1b, iters):
    """core/prior_raft.py:170-211.  L: the six leaves; pyr_*: four [B*N, 1, Hi, Wi] levels; g: `grids`; c1a / c1b: the
    coordinates entering the first iteration (free runs; a pinned run reads every iteration's from the pins)."""
    net_a, net_b, inp_a, inp_b, f1a, f2a = (L[k] for k in LEAVES)
    B, _, H8, W8 = net_a.shape
    dt = net_a.dtype
    c0 = po.coords_grid(B, H8, W8).to(dt)
    preds_a, preds_b = [], []
    for i in range(iters):
        run.i = i
        if run.pins is None:
            run.rec.append({})
            c1a, c1b = c1a.detach(), c1b.detach()                            # :171, :176
            run.rec[i]["c_a"], run.rec[i]["c_b"] = c1a, c1b
        else:
            c1a, c1b = run.pins[i]["c_a"].to(dt), run.pins[i]["c_b"].to(dt)
        flow_a = c1a - c0
        flow_b = c1b - c0
        if run.pins is None:
            flow_ba = po.flo_rotate(flow_b, g["b2a_w2c_8"], g["b2a_8"])      # :179
            run.rec[i]["flow_ba"] = flow_ba
        else:
            flow_ba = run.pins[i]["flow_ba"].to(dt)
        flaw_a = run.value("flaw_a", po.warp_groupwise_corr(f1a, f2a, c1a))                 # :173-174
        flaw_ba = run.value("flaw_ba", po.warp_groupwise_corr(f1a, f2a, c0 + flow_ba))      # :181-182
        own_a, cross_a = po.dccl_lookup(c1a, pyr_a, pyr_b, g["a2b_w2c_8"], g["b2a_8"])      # :185, :187
        own_b, cross_b = po.dccl_lookup(c1b, pyr_b, pyr_a, g["b2a_w2c_8"], g["a2b_8"])      # :186, :188
        na, nb, ia, ib = net_a, net_b, inp_a, inp_b
        if run.fault == "flaw_ba_detached":
            flaw_ba = flaw_ba.detach()
        if run.fault == "warp2_reads_conf_0_4":
            flaw_a, flaw_ba = _GradOfFirst.apply(flaw_a, flaw_ba)
        if run.fault == "cross_detached":
            cross_a = cross_a.detach()
        if run.fault == "d_inp_last_only" and i < iters - 1:
            ia, ib = ia.detach(), ib.detach()
        if run.fault == "hidden_not_handed_on" and i == 1:
            na = na.detach()
        corr_a = run.value("corr_a", own_a + cross_a)
        corr_b = run.value("corr_b", own_b + cross_b)
        net_a, mask_a, d_a = _update_a(run, na, ia, flow_a, corr_a, flaw_a, flow_ba, flaw_ba)
        net_b, mask_b, d_b = _update_b(run, nb, ib, corr_b, flow_b)
        c1a = c1a + d_a                                                      # :193-197
        c1b = c1b + d_b
        preds_a.append(po.upsample_flow(c1a - c0, mask_a))                   # :200-208
        preds_b.append(po.upsample_flow(c1b - c0, mask_b))
    return preds_a, preds_b


def evaluate(case: Case, inputs: dict, device, dtype, conv, pins: Optional[State] = None, fault: Optional[str] = None):
    """One forward + backward of `loop_body` on `device` in `dtype`.  Returns (gradients {name: tensor}: the LEAVES as d_<leaf>,
    the PYR levels as [B*N, Hi*Wi] rows, the update blocks' parameters under their own names; predictions; recorded state)."""
    B, H8, W8 = case.B, case.H8, case.W8
    dev = torch.device(device)
    g = grids(case, dev, dtype)                 # computed on the CPU in fp32, as the golden-pinned oracle does
    with torch.device(dev):                     # the oracle's factory calls (arange, linspace) follow the case's device
        mk = lambda t: t.to(device=dev, dtype=dtype).clone().requires_grad_(True)      # noqa: E731
        L = {k: mk(inputs[k]) for k in LEAVES}
        hs = [(H8 >> i, W8 >> i) for i in range(4)]
        pyr = {k: mk(inputs[k]) for k in PYR}
        lv = {t: [pyr[f"pyr_{t}{i}"].view(B * H8 * W8, 1, *hs[i]) for i in range(4)] for t in "ab"}
        p = {k: mk(v) for k, v in update_weights().items()}
        c0 = po.coords_grid(B, H8, W8).to(dtype)
        init = inputs["init_flow"].to(device=dev, dtype=dtype)
        c1a = c0 + init                                                                  # :162-165
        c1b = c0 + po.flo_rotate(init, g["a2b_w2c_8"], g["a2b_8"])
        run = _Run(p, conv, pins, fault)
        pa, pb = loop_body(run, L, lv["a"], lv["b"], g, c1a, c1b, case.iters)
        torch.autograd.backward(pa + pb, [s.to(device=dev, dtype=dtype) for s in inputs["seeds"]])
    grads = {"d_" + k: L[k].grad for k in LEAVES}
    grads.update({k: v.grad for k, v in pyr.items()})
    grads.update({k: v.grad for k, v in p.items()})
    return grads, [t.detach() for t in pa + pb], run.rec


def reference_and_model(case: Case, inputs: dict, pins: State, device):
    """(float64 pinned reference, float32 pinned rounding model, the reference's predictions)."""
    ref, preds, _ = evaluate(case, inputs, device, torch.float64, conv_plain, pins)
    model, _, _ = evaluate(case, inputs, device, torch.float32, conv_split, pins)
    return ref, model, preds


# ---------------------------------------------------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------------------------------------------------
def _capped_norm(err: torch.Tensor, cap: bool):
    """(norm of err, elements left out).  cap: the seam rule of the module docstring."""
    e = err.reshape(-1).abs()
    if not cap or e.numel() <= SEAM_CAP:
        return float(e.norm()), 0
    top, idx = torch.topk(e, SEAM_CAP)
    rest = e.clone()
    rest[idx] = 0
    rms = float(rest.norm()) / (e.numel() - SEAM_CAP) ** 0.5
    out = top > SEAM_FACTOR * rms
    n = int(out.sum())
    if n == 0:
        return float(e.norm()), 0
    rest[idx[~out]] = top[~out]
    return float(rest.norm()), n


def check(got: Dict[str, torch.Tensor], ref: Dict[str, torch.Tensor], model: Dict[str, torch.Tensor], model_ref=None):
    """-> (failures, {tensor: (err / bound, capped elements, E_t, bound / ||ref||)}); every tensor of `ref` must be in `got`.  model_ref: the
    reference the model's error E_t is taken against when it is not `ref` (the unpinned comparison of the host test)."""
    fails, report = [], {}
    model_ref = ref if model_ref is None else model_ref
    norms = {k: float(v.double().norm()) for k, v in ref.items()}
    scale = max(norms.values())
    for k, r in ref.items():
        r = r.double()
        if k not in got or got[k] is None:
            fails.append(f"{k}: no gradient")
            continue
        if tuple(got[k].shape) != tuple(r.shape):
            fails.append(f"{k}: shape {tuple(got[k].shape)}, expected {tuple(r.shape)}")
            continue
        cap = k in PYR
        e_model, _ = _capped_norm(model[k].double() - model_ref[k].double(), cap)
        bound = K_AGG * e_model + (ABS_TERM * scale if norms[k] <= ABS_TERM * scale else 0.0)
        d = got[k].double().to(r.device) - r
        if not bool(torch.isfinite(d).all()):
            fails.append(f"{k}: not finite")
            continue
        err, n_cap = _capped_norm(d, cap)
        ratio = err / bound if bound > 0 else (0.0 if err == 0 else float('inf'))
        report[k] = (ratio, n_cap, e_model / norms[k] if norms[k] > 0 else 0.0, bound / norms[k] if norms[k] > 0 else float('inf'))
        if err > bound:
            fails.append(f"{k}: |err| {err:.3e} > bound {bound:.3e} (x{ratio:.1f}; |ref| {norms[k]:.3e}, "
                         f"E_t {report[k][2]:.2e}, {n_cap} capped)")
    return fails, report


def worst(report, n=3) -> str:
    rows = sorted(((v[0], k, v[1]) for k, v in report.items()), reverse=True)[:n]
    capped = sum(v[1] for v in report.values())
    return ", ".join(f"{k} {r:.3f}" for r, k, _ in rows) + f"; {capped} capped"


def old_metric(got, ref) -> float:
    """What the end-to-end tests look at: the worst diff / (norm + 1e-3 * total) over the PARAMETER gradients."""
    names = [k for k in ref if k.startswith(("ODDC.", "update_block."))]
    total = sum(float(ref[k].double().pow(2).sum()) for k in names) ** 0.5
    return max(float((got[k].double().to(ref[k].device) - ref[k].double()).norm()) / (float(ref[k].double().norm()) + 1e-3 * total)
               for k in names)


def mean_epe(a, b) -> float:
    return float((a.double() - b.double().to(a.device)).norm(dim=1).mean())


# ---------------------------------------------------------------------------------------------------------------------
# the product's loop node, driven directly (GPU)
# ---------------------------------------------------------------------------------------------------------------------
class Harness:
    """train_loop.run_loop without the encoders: seeded leaves and hand-made pyramid triples (levels, token, PyramidGrad) in
    static device tensors (refreshed by `load`, so that a captured graph can be replayed on other inputs), the update blocks of a
    real PriOr_RAFT in train() + freeze_bn() with det_state_dict weights; the weight gradients arrive in the parameters' .grad
    (zeroed by `step`), straight from autograd (sink off) or through autograd.GradSink as train.train_step does it (sink on)."""

    def __init__(self, model, opt, case: Case):
        from prior_flow_amd import _lib
        from prior_flow_amd import autograd as ag
        self.model, self.opt, self.case = model, opt, case
        self.lib, self.ag = _lib.load(), ag
        dev = self.dev = next(model.parameters()).device
        B, H8, W8, it = case.B, case.H8, case.W8, case.iters
        N = B * H8 * W8
        z = lambda *s: torch.zeros(*s, device=dev)                                      # noqa: E731
        self.leaves = {k: z(B, 256 if k[0] == "f" else 128, H8, W8).requires_grad_(True) for k in LEAVES}
        self.levels = {t: [z(N, (H8 >> i) * (W8 >> i)) for i in range(4)] for t in "ab"}
        self.tokens = {t: z(1).requires_grad_(True) for t in "ab"}
        self.c1 = {t: z(B, 2, H8, W8) for t in "ab"}
        self.seeds = [z(B, 2, 8 * H8, 8 * W8) for _ in range(2 * it)]
        self.coords0 = ag._coords0(B, H8, W8, dev)
        _, self.g_a2b_8, self.g_b2a_8 = ag._grids(8 * H8, 8 * W8, dev)
        self.pg = None
        self.preds = None

    def load(self, inputs: dict):
        """Copies one seeded input set into the static tensors; c1a / c1b from init_flow as _train_forward_body forms them.
        Also zeroes the loop's workspace in place (its state at allocation): the model keeps ONE workspace per shape, and a
        run on the same inputs before this one leaves the RIGHT values in it -- a launch that reads a buffer before its producer
        has written it (a missed wait), or a write that no longer happens, would find them there and pass."""
        bufs = getattr(self.model, "_loop_bufs", None)
        with torch.no_grad():
            for S in ((bufs.a, bufs.b) if bufs is not None else ()):
                for v in S.values():
                    for t in (v if isinstance(v, list) else [v]):
                        t.zero_()
            for k in LEAVES:
                self.leaves[k].copy_(inputs[k])
            for t in "ab":
                for i in range(4):
                    self.levels[t][i].copy_(inputs[f"pyr_{t}{i}"])
            fl = inputs["init_flow"].to(self.dev).float().contiguous()
            self.c1["a"].copy_(self.coords0 + fl)
            self.c1["b"].copy_(self.coords0 + self.lib.flo_rotate(fl, self.g_b2a_8, self.g_a2b_8, torch.empty_like(fl)))
            for dst, src in zip(self.seeds, inputs["seeds"]):
                dst.copy_(src)

    def step(self, sink_on: bool):
        """zero the gradients, forward, backward[, sink flush] -- every launch of it can be captured into a graph."""
        from prior_flow_amd import train as tr
        from prior_flow_amd.train_loop import run_loop
        ag, model = self.ag, self.model
        self.opt.grad.zero_()
        for t in list(self.leaves.values()) + list(self.tokens.values()):
            t.grad = None
        if sink_on:
            sink = tr._grad_sink(self.opt)
            # begin() stays off silently when a parameter lacks a contiguous fp32 .grad, and PRIORFLOW_GRAD_SINK=0 switches it
            # off: the run would take the autograd route and still be reported as 'sink'
            assert sink.active, "the gradient sink did not start"
        else:
            sink = ag.SINK.for_device(self.dev.index)
            sink.active = False
        ag._TAPE.gates = {}                     # what train_forward sets
        ag._PACKS.clear()
        try:
            zr_a, zr_b = ag.fuse_zr(model.ODDC.gru, False), ag.fuse_zr(model.update_block.gru, False)
            self.pg = {t: ag.PyramidGrad() for t in "ab"}
            pyr = {t: (self.levels[t], self.tokens[t], self.pg[t]) for t in "ab"}
            L = self.leaves
            pa, pb = run_loop(model, self.lib, zr_a, zr_b, ag.gate_of, L["net_a"], L["net_b"], L["inp_a"], L["inp_b"], L["f1a"],
                              L["f2a"], pyr["a"], pyr["b"], self.coords0, self.c1["a"], self.c1["b"], self.g_a2b_8,
                              self.g_b2a_8, self.case.iters)
            self.preds = list(pa) + list(pb)
            torch.autograd.backward(self.preds, self.seeds)
            if sink_on:         # the deferred weight gradients went to the side stream, which the flush has to join
                assert model._loop_side_stream in sink.join_streams
        except BaseException:
            sink.abort()
            raise
        finally:
            ag._TAPE.gates = None
        if sink_on:
            sink.flush()

    def forget(self):
        """Drops every reference to the last step's autograd graph.  Needed between a warm-up step and a capture of `step` on the
        same leaves: a leaf's AccumulateGrad node is bound to the stream it was created on and lives as long as a graph that
        holds it, and the engine then synchronises THAT stream with the capturing one inside the capture; when that is the
        default stream (an eager step before the capture) the process dies in capture_end."""
        self.preds = self.pg = None
        for t in list(self.leaves.values()) + list(self.tokens.values()):
            t.grad = None

    def gradients(self) -> Dict[str, torch.Tensor]:
        """Every output of LoopFn.backward, named as `evaluate` names them (copies)."""
        out = {"d_" + k: v.grad.detach().clone() for k, v in self.leaves.items()}
        for t in "ab":
            for i, gl in enumerate(self.pg[t].g):
                out[f"pyr_{t}{i}"] = gl.detach().clone()
        for k, prm in self.model.named_parameters():
            if k.startswith(("ODDC.", "update_block.")):
                out[k] = prm.grad.detach().clone()
        return out

    def state(self) -> State:
        return state_from_buffers(self.model._loop_bufs, self.case)


@contextlib.contextmanager
def clean_tape():
    """Leaves autograd.SINK / _TAPE / _PACKS as a fresh process has them, whatever the body did: a failing case must not
    poison the next."""
    from prior_flow_amd import autograd as ag
    try:
        yield
    finally:
        ag._TAPE.gates = None
        ag._PACKS.clear()
        if torch.cuda.is_available():
            ag.SINK.for_device(torch.cuda.current_device()).abort()
