"""The head of a training step -- everything autograd._train_forward_body does before run_loop: both encoders, ContextSplit,
SplitBatch and the two correlation pyramids -- against float64 AT ITS SAVED STATE.  Helper of test_train_head_reference.py
(host) and test_hip_train_head.py (GPU); not a conftest, no test functions.  The tail of the tape has train_loop_ref.py; this
file follows it and takes `conv_split`, `split_round`, `check`, `worst`, `clean_tape`, K_AGG and ABS_TERM from it (`old_metric`
is the same formula over the encoders' names).

WHAT IS COMPARED.  `head` is oracle/priorflow_oracle.py's `encoder` / `_resblock` / `_norm` written out on a tap-matmul
convolution (`conv_taps`: one matmul per tap, stride by slicing the taps -- no library convolution runs in float64), then
tanh / relu of cnet's halves, fnet's four-way split and corr_volume + build_pyramid of both branches.  Forward: fm and the four
context tensors.  Backward: every fnet and cnet parameter gradient (94 tensors: 16 convolutions per encoder, 15 BatchNorm
layers in cnet, norm3 / downsample.1 counted once) for uniform [-1, 1] seeds on net_a, inp_a, net_b, inp_b, f1a, f2a and on
the eight pyramid levels.

WHAT IS PINNED.  Two correct runs in two precisions differ by far more than rounding where a pre-activation near zero flips a
ReLU mask.  So the reference takes every ReLU as x * (saved output > 0) of the run under test: the 13 norm + ReLU and the 6
relu(x + y) of each encoder and the relu that makes inp.  Nothing else is pinned: the statistics of InstanceNorm / BatchNorm,
tanh and the correlation volume are smooth.  A free run records its own ReLU outputs (the host test's "kernel").

WHERE THE TOLERANCE COMES FROM.  train_loop_ref.check, unchanged.  The ROUNDING MODEL is the same pinned graph in float32 in
which every convolution with more than 4 input channels rounds both operands to bf16 hi + bf16 lo in the forward, the
data-gradient and the weight-gradient pass (`conv_split`; a stride-2 convolution is the stride-1 one read at every second
position, so its backward is the stride-1 backward of the zero-stuffed gradient -- the product's route), the 3-channel 7x7
stems stay plain fp32 (pf_conv2d_small / pf_conv2d_wgrad_small are), and the volume and its two gradient GEMMs round both
operands with `split_round`.  For tensor t, E_t = ||model_t - ref_t|| / ||ref_t|| and the run under test must satisfy
        ||got_t - ref_t|| <= K_AGG * E_t * ||ref_t||   (+ ABS_TERM * max_t ||ref_t|| only where ||ref_t|| is below that term)
No element is left out of any tensor (there is no sampler in the head, so nothing like the loop's seam cap exists here).

CONDITION (asserted on the CPU, test_train_head_reference.py): K_AGG * E_t <= 1e-3 for every tensor of both cases, frozen and
batch-statistics BatchNorm -- the loop suite's figure, 20x below the 2e-2 of the end-to-end tests.  Measured: E_t <= 2.8e-5
for every gradient (K_AGG * E_t <= 2.3e-4) and <= 1.7e-5 for the forward tensors.

NAMED EXCEPTIONS (`zero_gradient_names`).  A convolution bias in front of a normalisation that subtracts the mean it has just
computed has a gradient of EXACTLY zero: the 15 biases of fnet in front of an InstanceNorm (all but fnet.conv2.bias), and with
batch statistics the 15 of cnet in front of a BatchNorm (all but cnet.conv2.bias).  The float64 reference holds rounding
residue there (1e-18 .. 1e-16 of the largest gradient's norm), E_t is residue over residue (1e8) and means nothing.  These
are the tensors `check` gives its absolute term: ||got|| <= K_AGG * ||model - ref|| + ABS_TERM * max_t ||ref_t||; both tests
assert that the tensors below that term are these and no others, so no live gradient is ever passed by it.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional

import torch
import torch.nn.functional as F

import golden_cases as gc
import priorflow_oracle as po
from train_loop_ref import ABS_TERM, K_AGG, check, clean_tape, conv_split, split_round, worst  # noqa: F401

LEAVES = ("net_a", "inp_a", "net_b", "inp_b", "f1a", "f2a")
PYR = tuple(f"pyr_{t}{i}" for t in "ab" for i in range(4))
FWD = ("fm", "net_a", "inp_a", "net_b", "inp_b")
BLOCKS = (("layer1.0.", 1), ("layer1.1.", 1), ("layer2.0.", 2), ("layer2.1.", 1), ("layer3.0.", 2), ("layer3.1.", 1))
N_PARAMS = 94                                   # asserted against model.named_parameters() by both tests


@dataclass(frozen=True)
class Case:
    name: str
    B: int
    H: int
    W: int
    seed: int = 1

    @property
    def H8(self):
        return self.H // 8

    @property
    def W8(self):
        return self.W // 8


# The smallest images train_forward accepts (>= 128, multiples of 8) at which the head still goes wrong.  EVEN: a live batch
# index in every per-image slice of the volume gradient, n = 512 needs no K padding.  RAGGED: ragged tiles at 68x108, 34x54 and
# 17x27, n = 459 takes the F.pad route (n4 = 460), the pyramid pools with floor (17x27 -> 8x13 -> 4x6 -> 2x3).
EVEN = Case("B2_128x256", 2, 128, 256)
RAGGED = Case("B1_136x216", 1, 136, 216)


# ---------------------------------------------------------------------------------------------------------------------
# seeded inputs, weights
# ---------------------------------------------------------------------------------------------------------------------
def images(case: Case):
    return gc.synthetic_pair(case.B, case.H, case.W)


def host_batches(case: Case):
    """img_f = [im1 | im2 | im1_B | im2_B] and img_c = [im1 | im1_B] as forward_with_grad forms them (the host test's inputs;
    the GPU test starts the reference from the batches pf_prepare_images wrote)."""
    i1, i2 = images(case)
    i1, i2 = 2 * (i1 / 255.0) - 1.0, 2 * (i2 / 255.0) - 1.0
    rot = po.img_rotate(torch.cat([i1, i2], 1), po.grids_for(case.H, case.W)["a2b"])
    i1b, i2b = rot[:, :3].contiguous(), rot[:, 3:].contiguous()
    return torch.cat([i1, i2, i1b, i2b], 0), torch.cat([i1, i1b], 0)


def make_seeds(case: Case) -> Dict[str, torch.Tensor]:
    """CPU fp32, uniform [-1, 1] as train_loop_ref.make_inputs draws them: the six leaves (NCHW) and the eight pyramid levels
    ([B*n, Hi*Wi] rows, the product's layout)."""
    B, H8, W8 = case.B, case.H8, case.W8
    gen = torch.Generator().manual_seed(case.seed)
    r = lambda *s: torch.rand(*s, generator=gen, dtype=torch.float32) * 2 - 1      # noqa: E731
    s = {k: r(B, 256 if k[0] == "f" else 128, H8, W8) for k in LEAVES}
    for t in "ab":
        for i in range(4):
            s[f"pyr_{t}{i}"] = r(B * H8 * W8, (H8 >> i) * (W8 >> i))
    return s


def weights_of(fnet, cnet) -> Dict[str, torch.Tensor]:
    """CPU copies of both encoders' state under the state_dict names, prefixed.  norm3 and downsample.1 are ONE module under two
    names: `head` reads downsample.1, the gradients are reported under named_parameters()'s name, norm3."""
    out = {}
    for pre, enc in (("fnet.", fnet), ("cnet.", cnet)):
        for k, v in enc.state_dict().items():
            if ".norm3." not in k:
                out[pre + k] = v.detach().cpu().clone()
    return out


_WEIGHTS: Dict[str, torch.Tensor] = {}


def det_weights() -> Dict[str, torch.Tensor]:
    """det_state_dict loaded into the parameter containers (which of the two aliases of norm3 wins is load_state_dict's
    business, as on the GPU) and read back."""
    if not _WEIGHTS:
        from prior_flow_amd.modules import BasicEncoder, state_dict_shapes
        sd = gc.det_state_dict(state_dict_shapes())
        encs = []
        for pre, kind in (("fnet.", "instance"), ("cnet.", "batch")):
            enc = BasicEncoder(256, kind)
            enc.load_state_dict({k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}, strict=True)
            encs.append(enc)
        _WEIGHTS.update(weights_of(*encs))
    return _WEIGHTS


def is_param(k: str) -> bool:
    return k.endswith((".weight", ".bias"))


def grad_name(k: str) -> str:
    return k.replace(".downsample.1.", ".norm3.")


def zero_gradient_names(names, bn_train: bool) -> set:
    """The convolution biases whose gradient is exactly zero (module docstring, NAMED EXCEPTIONS)."""
    conv_bias = lambda k: k.endswith(".bias") and ".norm" not in k          # noqa: E731
    out = {k for k in names if k.startswith("fnet.") and conv_bias(k) and k != "fnet.conv2.bias"}
    if bn_train:
        out |= {k for k in names if k.startswith("cnet.") and conv_bias(k) and k != "cnet.conv2.bias"}
    return out


def below_abs_term(ref) -> set:
    """The tensors of `ref` to which `check` applies its absolute term."""
    norms = {k: float(v.double().norm()) for k, v in ref.items()}
    scale = max(norms.values())
    return {k for k, n in norms.items() if n <= ABS_TERM * scale}


# ---------------------------------------------------------------------------------------------------------------------
# convolution
# ---------------------------------------------------------------------------------------------------------------------
def conv_taps(x, w, b, pad, stride=1):
    """F.conv2d(x, w, b, stride=stride, padding=pad) as one matmul per tap in x's dtype on x's device (train_loop_ref.conv_taps
    with a stride: tap (ky, kx) reads xp[:, ky:ky + s*Ho:s, kx:kx + s*Wo:s])."""
    co, ci, kh, kw = w.shape
    B, _, H, W = x.shape
    s = stride
    Ho, Wo = (H + 2 * pad[0] - kh) // s + 1, (W + 2 * pad[1] - kw) // s + 1
    xp = F.pad(x.permute(0, 2, 3, 1), (0, 0, pad[1], pad[1], pad[0], pad[0]))
    wt = w.permute(2, 3, 1, 0)
    y = None
    for ky in range(kh):
        for kx in range(kw):
            t = xp[:, ky:ky + s * Ho:s, kx:kx + s * Wo:s, :].reshape(-1, ci) @ wt[ky, kx]
            y = t if y is None else y + t
    if b is not None:
        y = y + b
    return y.view(B, Ho, Wo, co).permute(0, 3, 1, 2).contiguous()


def conv_plain(x, w, b, pad, stride=1):
    return conv_taps(x, w, b, pad, stride)


def conv_model(x, w, b, pad, stride=1):
    """The rounding model's convolution: bf16 hi + lo operands in all three passes where the product runs pf_conv2d (more than 4
    input channels), plain fp32 where it runs pf_conv2d_small (the 3-channel stems).  Stride 2 (3x3 pad 1 / 1x1 pad 0 on even
    maps): out[p] = stride-1 out[2p], whose backward is the stride-1 backward of the zero-stuffed gradient -- HipConvS2's."""
    if x.dtype == torch.float32 and x.shape[1] > 4:
        y = conv_split(x, w, b, pad)
        return y if stride == 1 else y[:, :, ::stride, ::stride]
    return conv_taps(x, w, b, pad, stride)


# ---------------------------------------------------------------------------------------------------------------------
# seeded faults of the backward (host test): none of them changes a forward value
# ---------------------------------------------------------------------------------------------------------------------
FAULTS = ("df2_from_dv", "df1_unscaled", "image1_reads_image0", "last_k_dropped", "s2_dx_last_row", "s2_bias_half",
          "inorm_no_gx_term", "bn_dgamma_no_mask", "add_relu_one_input", "split_swapped", "tanh_1_minus_t", "norm3_twice",
          "bn_dbeta_over_n")
FAULT_NEEDS_BN_TRAIN = ("bn_dbeta_over_n",)
FAULT_NEEDS_FROZEN = ("bn_dgamma_no_mask",)


class _GradEdit(torch.autograd.Function):
    """x -> x; the gradient goes through `fn`."""

    @staticmethod
    def forward(ctx, x, fn):
        ctx.fn = fn
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return ctx.fn(g), None


class _TanhFault(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        t = torch.tanh(x)
        ctx.save_for_backward(t)
        return t

    @staticmethod
    def backward(ctx, g):
        t, = ctx.saved_tensors
        return g * (1 - t)


class _INormFault(torch.autograd.Function):
    """InstanceNorm whose backward lacks the mean(g * xhat) term: dx = rstd * (g - mean(g))."""

    @staticmethod
    def forward(ctx, x):
        mu = x.mean(dim=(2, 3), keepdim=True)
        std = torch.sqrt(x.var(dim=(2, 3), unbiased=False, keepdim=True) + 1e-5)
        ctx.save_for_backward(1 / std)
        return (x - mu) / std                       # the clean run's expression: no forward value changes

    @staticmethod
    def backward(ctx, g):
        rstd, = ctx.saved_tensors
        return rstd * (g - g.mean(dim=(2, 3), keepdim=True))


class _PinnedRelu(torch.autograd.Function):
    """x * (saved output > 0).  The backward is relu's own kernel on the saved output, g where it is positive: the same values
    as g * mask in the memory layout relu's backward gives them, so that the reductions behind it add in the same order and a
    reference pinned to its own state is the free one bit for bit."""

    @staticmethod
    def forward(ctx, x, out):
        out = out.to(x.dtype)
        ctx.save_for_backward(out)
        return x * (out > 0).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        out, = ctx.saved_tensors
        return torch.ops.aten.threshold_backward(g, out, 0), None


class _Volume(torch.autograd.Function):
    """V[b] = F1[b] F2[b]^T / sqrt(C) with F = the [n, C] rows of a feature map (po.corr_volume), and its two gradient GEMMs
    d F1 = dV F2 / sqrt(C), d F2 = dV^T F1 / sqrt(C) written out, so that the rounding model can round their operands
    (`rnd`: split_round of both operands of all three GEMMs) and a fault can be seeded into them."""

    @staticmethod
    def forward(ctx, f1, f2, rnd, fault):
        B, C, H, W = f1.shape
        r = split_round if rnd else (lambda t: t)
        F1 = r(f1.reshape(B, C, H * W).transpose(1, 2))
        F2 = r(f2.reshape(B, C, H * W).transpose(1, 2))
        ctx.save_for_backward(F1, F2)
        ctx.cfg = (f1.shape, rnd, fault)
        return (F1 @ F2.transpose(1, 2)) * (1.0 / math.sqrt(C))

    @staticmethod
    def backward(ctx, dv):
        F1, F2 = ctx.saved_tensors
        (B, C, H, W), rnd, fault = ctx.cfg
        n = H * W
        s = 1.0 / math.sqrt(C)
        g = split_round(dv) if rnd else dv
        gt = g.transpose(1, 2)
        if fault == "df2_from_dv":
            gt = g
        if fault == "image1_reads_image0" and B > 1:
            F1, F2 = F1.clone(), F2.clone()
            F1[1], F2[1] = F1[0], F2[0]
        if fault == "last_k_dropped":               # column n4 - 1 of the padded K: a pad column when n % 4 != 0
            k = (n + 3) // 4 * 4 - 1
            if k < n:
                g, gt = g.clone(), gt.clone()
                g[:, :, k] = 0
                gt[:, :, k] = 0
        d1 = (g @ F2) * (1.0 if fault == "df1_unscaled" else s)
        d2 = (gt @ F1) * s
        back = lambda d: d.transpose(1, 2).reshape(B, C, H, W)      # noqa: E731
        return back(d1), back(d2), None, None


# ---------------------------------------------------------------------------------------------------------------------
# the head graph
# ---------------------------------------------------------------------------------------------------------------------
class _Run:
    """One evaluation: the parameters, the convolution, the pins (None: free), the record of ReLU outputs being written and
    the running statistics batch-statistics BatchNorm should leave."""

    def __init__(self, p, conv, pins, bn_train, fault):
        self.p, self.conv, self.pins, self.bn_train, self.fault = p, conv, pins, bn_train, fault
        self.rec: Dict[str, torch.Tensor] = {}
        self.stats: Dict[str, torch.Tensor] = {}

    def cv(self, name, x, pad, stride=1):
        w, b = self.p[name + ".weight"], self.p[name + ".bias"]
        if stride == 2 and x.shape[1] > 4 and self.fault == "s2_dx_last_row":
            def drop(g):
                g = g.clone()
                g[:, :, -1] = 0
                return g
            x = _GradEdit.apply(x, drop)
        if stride == 2 and x.shape[1] > 4 and self.fault == "s2_bias_half":
            y = self.conv(x, w, None, (pad, pad), stride)

            def half(g):
                g = g.clone()
                g[:, :, 1::2] = 0
                return g
            return y + _GradEdit.apply(b.view(1, -1, 1, 1).expand_as(y), half)
        return self.conv(x, w, b, (pad, pad), stride)

    def relu(self, key, x):
        if self.pins is not None:
            return _PinnedRelu.apply(x, self.pins[key])
        y = F.relu(x)
        self.rec[key] = y.detach()
        return y

    def norm(self, name, x, kind):
        """po._norm; with bn_train nn.BatchNorm2d in training mode (batch statistics over the whole batch) and the running
        statistics it leaves: momentum 0.1, unbiased variance, num_batches_tracked + 1."""
        if kind == "instance":
            if self.fault == "inorm_no_gx_term":
                return _INormFault.apply(x)
            mu = x.mean(dim=(2, 3), keepdim=True)
            var = x.var(dim=(2, 3), unbiased=False, keepdim=True)
            return (x - mu) / torch.sqrt(var + 1e-5)
        p = self.p
        w, b = p[name + ".weight"], p[name + ".bias"]
        rm, rv = p[name + ".running_mean"], p[name + ".running_var"]
        if self.fault == "norm3_twice" and name.endswith("downsample.1"):
            w, b = (_GradEdit.apply(t, lambda g: g * 2.0) for t in (w, b))
        if not self.bn_train:
            scale = w / torch.sqrt(rv + 1e-5)
            return (x - rm.view(1, -1, 1, 1)) * scale.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)
        n = x.shape[0] * x.shape[2] * x.shape[3]
        if self.fault == "bn_dbeta_over_n":
            b = _GradEdit.apply(b, lambda g: g / n)
        mu = x.mean(dim=(0, 2, 3), keepdim=True)
        var = x.var(dim=(0, 2, 3), unbiased=False, keepdim=True)
        with torch.no_grad():
            self.stats[name + ".running_mean"] = 0.9 * rm + 0.1 * mu.reshape(-1)
            self.stats[name + ".running_var"] = 0.9 * rv + 0.1 * var.reshape(-1) * (n / (n - 1))
            self.stats[name + ".num_batches_tracked"] = p[name + ".num_batches_tracked"] + 1
        return (x - mu) / torch.sqrt(var + 1e-5) * w.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)

    def norm_relu(self, name, x, kind):
        y = self.norm(name, x, kind)
        out = self.relu(name, y)
        if self.fault == "bn_dgamma_no_mask" and kind == "batch" and not self.bn_train:
            # d gamma = sum g * xhat over ALL positions: add the unmasked part, a term whose value is zero
            w = self.p[name + ".weight"]
            rm, rv = self.p[name + ".running_mean"], self.p[name + ".running_var"]
            xh = ((x - rm.view(1, -1, 1, 1)) / torch.sqrt(rv + 1e-5).view(1, -1, 1, 1)).detach()
            dead = (out.detach() <= 0).to(x.dtype)
            t = xh * dead * w.view(1, -1, 1, 1)
            out = out + (t - t.detach())
        return out


def _resblock(run: _Run, pre, x, kind, stride):
    """po._resblock (core/extractor.py:8-47)."""
    y = run.norm_relu(pre + "norm1", run.cv(pre + "conv1", x, 1, stride), kind)
    y = run.norm_relu(pre + "norm2", run.cv(pre + "conv2", y, 1), kind)
    if stride != 1:
        x = run.norm(pre + "downsample.1", run.cv(pre + "downsample.0", x, 0, stride), kind)      # == norm3
    if run.fault == "add_relu_one_input":
        y = _GradEdit.apply(y, torch.zeros_like)
    return run.relu(pre + "out", x + y)


def _encoder(run: _Run, pre, x, kind):
    """po.encoder (core/extractor.py:98-158), dropout off."""
    x = run.norm_relu(pre + "norm1", run.cv(pre + "conv1", x, 3, 2), kind)
    for blk, stride in BLOCKS:
        x = _resblock(run, pre + blk, x, kind, stride)
    return run.cv(pre + "conv2", x, 0)


def relu_keys() -> List[str]:
    ks = []
    for pre in ("fnet.", "cnet."):
        ks.append(pre + "norm1")
        for blk, _ in BLOCKS:
            ks += [pre + blk + "norm1", pre + blk + "norm2", pre + blk + "out"]
    return ks + ["cnet.inp"]


def head(p, img_f, img_c, B, dtype, conv, pins=None, bn_train=False, fault=None):
    """core/prior_raft.py:133-159 on prepared batches: -> (outputs {fm, net_a, inp_a, net_b, inp_b, f1a, f2a, pyr_a, pyr_b (four
    [B*n, 1, Hi, Wi] levels each)}, the _Run with the ReLU record and the running statistics).  p: state_dict names -> tensors
    of `dtype` on the device of the images."""
    run = _Run(p, conv, pins, bn_train, fault)
    rnd = conv is conv_model and dtype == torch.float32
    cn = _encoder(run, "cnet.", img_c.to(dtype), "batch")
    t = _TanhFault.apply(cn[:, :128]) if fault == "tanh_1_minus_t" else torch.tanh(cn[:, :128])
    r = run.relu("cnet.inp", cn[:, 128:])
    fm = _encoder(run, "fnet.", img_f.to(dtype), "instance")
    out = dict(fm=fm, net_a=t[:B], inp_a=r[:B], net_b=t[B:], inp_b=r[B:])
    fs = fm
    if fault == "split_swapped":
        fs = _GradEdit.apply(fm, lambda g: torch.cat([g[:B], g[2 * B:3 * B], g[B:2 * B], g[3 * B:]], 0))
    f1a, f2a, f1b, f2b = fs[:B], fs[B:2 * B], fs[2 * B:3 * B], fs[3 * B:]
    out.update(f1a=f1a, f2a=f2a)
    H8, W8 = fm.shape[2:]
    for tag, (f1, f2) in (("a", (f1a, f2a)), ("b", (f1b, f2b))):
        v = _Volume.apply(f1, f2, rnd, fault)
        out["pyr_" + tag] = po.build_pyramid(v.reshape(B, H8, W8, H8, W8))
    return out, run


def evaluate(case: Case, weights, img_f, img_c, seeds, device, dtype, conv, pins=None, bn_train=False, fault=None):
    """One forward + backward of `head` on `device` in `dtype` -> (forward {FWD}, gradients {parameter name as
    named_parameters() has it}, ReLU record, running statistics)."""
    dev = torch.device(device)
    B = case.B
    p = {}
    for k, v in weights.items():
        v = v.to(dev)
        p[k] = v.to(dtype).clone().requires_grad_(True) if is_param(k) else (v.to(dtype) if v.dtype.is_floating_point else v)
    out, run = head(p, img_f.to(dev), img_c.to(dev), B, dtype, conv, pins, bn_train, fault)
    roots = [out[k] for k in LEAVES] + out["pyr_a"] + out["pyr_b"]
    gs = [seeds[k].to(device=dev, dtype=dtype) for k in LEAVES]
    gs += [seeds[k].to(device=dev, dtype=dtype).view(r.shape) for k, r in zip(PYR, out["pyr_a"] + out["pyr_b"])]
    torch.autograd.backward(roots, gs)
    grads = {grad_name(k): v.grad for k, v in p.items() if is_param(k)}
    assert len(grads) == N_PARAMS and all(g is not None for g in grads.values())
    return {k: out[k].detach() for k in FWD}, grads, run.rec, run.stats


def reference_and_model(case, weights, img_f, img_c, seeds, pins, device, bn_train=False):
    """(float64 pinned reference, float32 pinned rounding model), each (forward, gradients, -, running statistics)."""
    ref = evaluate(case, weights, img_f, img_c, seeds, device, torch.float64, conv_plain, pins, bn_train)
    model = evaluate(case, weights, img_f, img_c, seeds, device, torch.float32, conv_model, pins, bn_train)
    return ref, model


def old_metric(got, ref) -> float:
    """What the end-to-end tests look at: the worst diff / (norm + 1e-3 * total) over the parameter gradients."""
    total = sum(float(v.double().pow(2).sum()) for v in ref.values()) ** 0.5
    return max(float((got[k].double().to(v.device) - v.double()).norm()) / (float(v.double().norm()) + 1e-3 * total)
               for k, v in ref.items())


GROUPS = ("fnet convs", "cnet convs", "cnet norms")


def group_of(k: str) -> str:
    if k.startswith("fnet."):
        return GROUPS[0]
    return GROUPS[2] if ".norm" in k else GROUPS[1]


def by_group(report, col=0, skip=()) -> str:
    """worst report column (0: err / bound, 2: E_t) per group of parameter gradients; `skip`: names left out (E_t of a
    gradient that is exactly zero is residue over residue)."""
    out = []
    for g in GROUPS:
        rows = [(v[col], k) for k, v in report.items() if k.startswith(("fnet.", "cnet.")) and k not in skip and group_of(k) == g]
        if rows:
            v, k = max(rows)
            out.append(f"{g} {v:.2e} ({k})")
    return "; ".join(out)


# ---------------------------------------------------------------------------------------------------------------------
# the correlation node alone (GPU): float64 d f1 / d f2 with the two bounds of conv_launches
# ---------------------------------------------------------------------------------------------------------------------
def volume_grad_fp64(f1, f2, level_grads, B, H, W):
    """d f1 = dV f2 / sqrt(C), d f2 = dV^T f1 / sqrt(C) in float64 on the tensors' device, dV = g0 + g1 / 4 + g2 / 16 + g3 / 64
    over the parents that exist (build_pyramid's floor pooling; elem_launches.ref_pyramid_bwd's form), each with the
    per-element and the aggregate bound of conv_launches for a bf16x3 GEMM of K = n products:

        |err| <= C_ELEM * (U_PROD[bf16x3] + (K + 3 + 1) * 2^-24) * A        A = sum_j Dabs_j |f_jc| / sqrt(C)
        |err| <= K_AGG * (U_PROD[bf16x3] + sqrt(K) * 2^-23 + (3 + 1) * 2^-24) * R   R = sqrt(sum_j (Dabs_j f_jc)^2) / sqrt(C)

    K * 2^-24 / sqrt(K) * 2^-23: the fp32 accumulator (conv_launches).  + 3: the three fp32 additions of pf_pyramid_bwd, each at
    most 2^-24 of Dabs = |g0| + |g1| / 4 + |g2| / 16 + |g3| / 64 (the factors are powers of two: exact), which is why A and R
    are taken over Dabs and not |dV|.  + 1: one rounding for the 1 / sqrt(C) scale of the epilogue.
    -> {"d_f1": (ref, tol_elem, tol_agg), "d_f2": ...}, NCHW."""
    from conv_launches import C_ELEM, U_PROD
    n = H * W
    C = f1.shape[1]
    g = [t.double().view(B, n, H >> i, W >> i) for i, t in enumerate(level_grads)]
    dv, dabs = g[0].clone(), g[0].abs()
    for i in (1, 2, 3):
        hi, wi = H >> i, W >> i
        up = g[i].repeat_interleave(1 << i, 2).repeat_interleave(1 << i, 3) * 0.25 ** i      # [B, n, hi << i, wi << i]
        dv[:, :, :hi << i, :wi << i] += up
        dabs[:, :, :hi << i, :wi << i] += up.abs()
    dv, dabs = dv.view(B, n, n), dabs.view(B, n, n)
    s = 1.0 / math.sqrt(C)
    rows = lambda f: f.double().reshape(B, C, n).transpose(1, 2)            # noqa: E731
    back = lambda d: d.transpose(1, 2).reshape(B, C, H, W)                  # noqa: E731
    u = 2.0 ** -24
    ue = C_ELEM * (U_PROD[1] + (n + 3 + 1) * u)
    ua = K_AGG * (U_PROD[1] + math.sqrt(n) * 2 * u + (3 + 1) * u)
    out = {}
    for name, d, da, f in (("d_f1", dv, dabs, rows(f2)), ("d_f2", dv.transpose(1, 2), dabs.transpose(1, 2), rows(f1))):
        out[name] = (back(d @ f * s), back(da @ f.abs() * s * ue), back(torch.sqrt(da.pow(2) @ f.pow(2)) * s * ua))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the product's head, driven through autograd.train_forward (GPU)
# ---------------------------------------------------------------------------------------------------------------------
class Harness:
    """autograd.train_forward(model, i1, i2, iters=1) with train_loop.run_loop replaced by a stub that hands back what it was
    given, so the side stream, _prepack_encoders, the tape's WeightGates and pf_prepare_images are the product's.  Recording
    wrappers around ag.encoder_forward, ag._norm and ag.HipAddRelu collect the img_f / img_c the run produced and every ReLU
    output (the pins).  `monkeypatch` is pytest's: everything is undone with the test."""

    def __init__(self, model, opt, case: Case, monkeypatch):
        from prior_flow_amd import autograd as ag
        from prior_flow_amd import train_loop
        self.model, self.opt, self.case, self.ag = model, opt, case, ag
        self.dev = next(model.parameters()).device
        self.rec: Dict[str, torch.Tensor] = {}
        self.given: Optional[dict] = None
        self.fm = self.img_f = self.img_c = None
        names = {id(m): k for k, m in model.named_modules()}
        state = {"pre": None, "blk": 0}
        h = self
        enc_fwd, norm, add_relu = ag.encoder_forward, ag._norm, ag.HipAddRelu

        def encoder_forward(enc, x):
            state["pre"], state["blk"] = names[id(enc)] + ".", 0
            if enc is model.cnet:
                h.img_c = x.detach().clone()
            else:
                h.img_f = x.detach().clone()
            y = enc_fwd(enc, x)
            if enc is model.fnet:
                h.fm = y
            return y

        def _norm(m, x, relu=False):
            y = norm(m, x, relu)
            if relu:
                h.rec[names[id(m)]] = y.detach().clone()
            return y

        class AddRelu:
            @staticmethod
            def apply(x, y):
                out = add_relu.apply(x, y)
                h.rec[state["pre"] + BLOCKS[state["blk"]][0] + "out"] = out.detach().clone()
                state["blk"] += 1
                return out

        def run_loop(model_, lib, zr_a, zr_b, gate_of, net_a, net_b, inp_a, inp_b, f1a, f2a, pyr_a, pyr_b, *rest):
            h.given = dict(net_a=net_a, inp_a=inp_a, net_b=net_b, inp_b=inp_b, f1a=f1a, f2a=f2a, pyr_a=pyr_a, pyr_b=pyr_b)
            return h.given

        monkeypatch.setattr(ag, "encoder_forward", encoder_forward)
        monkeypatch.setattr(ag, "_norm", _norm)
        monkeypatch.setattr(ag, "HipAddRelu", AddRelu)
        monkeypatch.setattr(train_loop, "run_loop", run_loop)
        monkeypatch.setenv("PRIORFLOW_TRAIN_LOOP", "1")
        monkeypatch.setenv("PRIORFLOW_GRAD_SINK", "1")
        i1, i2 = images(case)
        self.i1, self.i2 = i1.to(self.dev), i2.to(self.dev)
        self.seeds = {k: v.to(self.dev) for k, v in make_seeds(case).items()}

    def params(self):
        return [(k, p) for k, p in self.model.named_parameters() if k.startswith(("fnet.", "cnet."))]

    def step(self, sink_on: bool, zero: bool = True):
        """[zero the gradients,] forward, seeded level gradients into the pyramid accumulators, backward on the six leaves and
        the two tokens[, sink flush]."""
        from prior_flow_amd import train as tr
        ag = self.ag
        if zero:
            self.opt.grad.zero_()
        if sink_on:
            sink = tr._grad_sink(self.opt)
            assert sink.active, "the gradient sink did not start"
        else:
            sink = ag.SINK.for_device(self.dev.index)
            sink.active = False
        self.rec.clear()
        try:
            g = ag.train_forward(self.model, self.i1, self.i2, iters=1)
            assert g is self.given, "train_forward did not reach the loop"
            for t in "ab":
                levels, _, acc = g["pyr_" + t]
                for i, buf in enumerate(acc.buffers(levels)):
                    buf.copy_(self.seeds[f"pyr_{t}{i}"])
            toks = [g["pyr_a"][1], g["pyr_b"][1]]
            torch.autograd.backward([g[k] for k in LEAVES] + toks, [self.seeds[k] for k in LEAVES] + [torch.zeros_like(t) for t in toks])
        except BaseException:
            sink.abort()
            raise
        if sink_on:
            sink.flush()
        torch.cuda.synchronize()

    def forward(self) -> Dict[str, torch.Tensor]:
        out = {k: self.given[k].detach().clone() for k in FWD[1:]}
        out["fm"] = self.fm.detach().clone()
        return out

    def gradients(self) -> Dict[str, torch.Tensor]:
        return {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in self.params()}

    def pins(self) -> Dict[str, torch.Tensor]:
        pins = dict(self.rec)
        pins["cnet.inp"] = torch.cat([self.given["inp_a"], self.given["inp_b"]], 0).detach()
        return pins
