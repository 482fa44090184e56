"""Every pf_conv2d launch the product makes, replayed against a float64 reference (helper of test_hip_conv_launches.py and
test_conv_launch_reference.py; not a conftest).

  signature(lib, descs, B, H8, W8)   what decides the code a launch runs: precision, stride, kernel shape, epilogue, the
                                     planner's tile / roles, groups, operand and output forms, options.  Host logic only.
  Recorder                           context manager around PfLib.conv2d (the one Python entry to pf_conv2d): the signature,
                                     geometry and descriptor layout of every launch, in order.
  build_case(lib, launch, B, H, W)   fresh seeded buffers with the recorded layout (same ld / off / lds, sentinels outside
                                     the columns a launch may write), descriptors ready for lib.conv2d.
  reference(case)                    the same convolutions in float64 with per-element error bounds (see TOLERANCES).
  check_case(case, ref)              compares every output form, the fused statistics and the sentinels; returns failures.
  relation / reachable / witness     the plans a recorded layout reaches over the image sizes and batches the product supports
                                     (GRID), and the geometry at which to replay each of them.  Host logic only.

TOLERANCES.  For one output element v = b + sum_k x_k w_k (+ pre) let
    A = sum_k |x_k w_k| + |b| + |pre|        (what a worst-case rounding analysis multiplies)
    R = sqrt(sum_k (x_k w_k)^2 + b^2 + pre^2) (the scale of a random walk of independent per-product errors)
and K = kh * kw * cin.  Two bounds must hold for every element:
  * per element, |err| <= C_ELEM * u_e * A: a worst-case bound.  u_e = U_PROD + K * 2^-24: U_PROD per product
    (bf16x3: hi*hi + hi*lo + lo*hi drops lo*lo and the rounding of lo, each <= 2^-16 |x w|; fp32: one rounding 2^-24;
    fp16 against fp16-rounded operands: exact products) plus K fp32 additions of the accumulator.  Any dropped tap, wrong
    offset or edge, stale tile or wrong epilogue moves an element by a whole tap's worth, far beyond it.
  * aggregate, max |err| / R <= K_AGG * u_a, u_a = U_PROD + sqrt(K) * 2^-23: the per-product errors and the K roundings of
    the accumulator have random signs, so they add like a random walk of R's scale (sqrt(K) steps of at most 2^-24 of a partial
    sum of size <= R in fp32).  This is the tight one: a bf16x3 kernel that loses the hi*lo pass or runs one bf16 pass errs
    by ~2^-9 R (test_conv_launch_reference.py proves both fail), an fp16 conv whose operands were not rounded as the header
    says by ~2^-12 R.
Both bounds go through the epilogue: ReLU, sigmoid and tanh are 1-Lipschitz, `scale` multiplies them by |scale|, r*h by |h|,
(1-z) h + z q by z; the fp32 epilogue arithmetic adds a few ulp of the magnitudes involved (EPS_EPI) and the device expf / rcp
of the fast sigmoid / tanh an absolute 2^-20 (EPS_TRANS: a few ulp of values <= 1).  An output held only as a bf16 twin
(hi + lo, 16 significant bits) or an f16 map adds its own representation error, 2^-16 |v| resp. 2^-11 |v| + 2^-25.
"""
from __future__ import annotations

import contextlib
import math
from dataclasses import dataclass, field
from typing import Dict, List

import torch

EPI_NAMES = {0: "LINEAR", 1: "RELU", 2: "GRU_ZR", 3: "GRU_Q", 4: "TANH_RELU", 5: "RELU_RES", 6: "MASK", 7: "ADD"}
PREC_NAMES = {0: "fp32", 1: "bf16x3", 2: "f16"}
PTR_FIELDS = ("in0", "in1", "weight", "bias", "out", "h", "z", "aux_out", "in_scale", "in_shift", "stats_out", "in0_split",
              "in1_split", "out_split", "aux_split", "zeros", "pre")
INT_FIELDS = ("ld0", "off0", "c0", "ld1", "off1", "c1", "ld_out", "off_out", "cout", "kh", "kw", "epilogue", "ld_h", "ld_z",
              "ld_aux", "precision", "stride", "in_relu", "lds0", "lds1", "lds_out", "lds_aux", "zeros_bytes", "ld_pre",
              "off_pre", "save_gates", "co_groups")

C_ELEM, K_AGG = 4.0, 8.0
U_PROD = {0: 2.0 ** -24, 1: 2.0 ** -16, 2: 0.0}
EPS_EPI = 2.0 ** -22
EPS_TRANS = 2.0 ** -20
SENT_F32 = -1234.5                   # fp32 sentinel of output / aux columns a launch must not write
SENT_IN = 3.0e4                      # input columns outside the slice a launch reads: a wrong offset shows at once
SENT_BF16 = -77.0                    # sentinel of twin / map columns outside the written slice (exact in bf16 and fp16)


def _u_elem(prec, K):
    return U_PROD[prec] + K * 2.0 ** -24


def _u_agg(prec, K):
    return U_PROD[prec] + math.sqrt(K) * 2.0 ** -23


# ---------------------------------------------------------------------------------------------------------------------
# signature
# ---------------------------------------------------------------------------------------------------------------------
def _layout(d) -> dict:
    """The plain-data copy of one descriptor: every int field and which pointers are set (and the aliasing of out and h)."""
    g = {k: int(getattr(d, k)) for k in INT_FIELDS}
    g["scale"] = float(d.scale)
    for k in PTR_FIELDS:
        g["has_" + k] = bool(getattr(d, k))
    out, h = getattr(d, "out") or 0, getattr(d, "h") or 0
    g["alias_h"] = bool(out and h and h == out + 4 * d.off_out and d.ld_h == d.ld_out)
    return g


def _form(f32: bool, split: bool, prec: int) -> str:
    parts = (["fp32"] if f32 else []) + ([("f16map" if prec == 2 else "twin")] if split else [])
    return "+".join(parts) or "-"


def group_signature(g: dict) -> tuple:
    prec = g["precision"]
    opts = []
    if g["has_in_scale"]:
        opts.append("in_scale" + ("+relu" if g["in_relu"] else ""))
    for name, key in (("stats", "has_stats_out"), ("pre", "has_pre"), ("save_gates", "save_gates"), ("out=h", "alias_h")):
        if g[key]:
            opts.append(name)
    if g["scale"] != 1.0:
        opts.append("scale!=1")
    return (EPI_NAMES[g["epilogue"]],
            "in0:" + _form(g["has_in0"], g["has_in0_split"], prec),
            "in1:" + (_form(g["has_in1"], g["has_in1_split"], prec) if g["c1"] > 0 else "-"),
            "out:" + _form(g["has_out"], g["has_out_split"], prec),
            "aux:" + _form(g["has_aux_out"], g["has_aux_split"], prec),
            tuple(opts))


def plan(lib, descs, B, H8, W8):
    """(pf_conv2d_tile, pf_conv2d_roles) of a launch -- host arithmetic over the descriptors, no GPU."""
    arr = (type(descs[0]) * len(descs))(*descs)
    return (int(lib._dll.pf_conv2d_tile(arr, len(descs), B, H8, W8)), int(lib._dll.pf_conv2d_roles(arr, len(descs), B, H8, W8)))


def signature_of_layouts(tile_roles, groups: List[dict]) -> tuple:
    g0 = groups[0]
    return (PREC_NAMES[g0["precision"]], "s%d" % g0["stride"], "%dx%d" % (g0["kh"], g0["kw"]),
            "tile%d" % tile_roles[0], "roles%d" % tile_roles[1], "groups%d" % len(groups), "co%d" % g0["co_groups"],
            tuple(group_signature(g) for g in groups))


def signature(lib, descs, B, H8, W8) -> tuple:
    """Hashable description of one pf_conv2d launch (see the module docstring); uses the host planners only."""
    return signature_of_layouts(plan(lib, descs, B, H8, W8), [_layout(d) for d in descs])


def sig_str(sig) -> str:
    head = " ".join(sig[:7])
    groups = " | ".join(" ".join(x for x in (gs[0],) + gs[1:5] if not x.endswith(":-")) + ("" if not gs[5] else " [" + ",".join(gs[5]) + "]")
                        for gs in sig[7])
    return f"{head}  {groups}"


# ---------------------------------------------------------------------------------------------------------------------
# recorder
# ---------------------------------------------------------------------------------------------------------------------
@dataclass
class Launch:
    sig: tuple
    B: int
    H: int
    W: int
    groups: List[dict]
    path: str = ""
    image: tuple = None                # (B_img, H_img, W_img) of the product run the launch was recorded in


class Recorder(contextlib.AbstractContextManager):
    """Wraps PfLib.conv2d on the class: every launch is recorded, then runs as before.  Enter it before the model or
    engine is built (a bound method cached by one of them would otherwise escape)."""

    def __init__(self, path: str = "", image: tuple = None):
        self.path = path
        self.image = image             # the image geometry (B, H, W) of the path being recorded (see relation)
        self.launches: List[Launch] = []

    def __enter__(self):
        from prior_flow_amd import _lib
        self._cls = _lib.PfLib
        orig = self._orig = _lib.PfLib.conv2d
        rec = self

        def conv2d(lib, descs, B, H8, W8, like):
            groups = [_layout(d) for d in descs]
            rec.launches.append(Launch(signature_of_layouts(plan(lib, list(descs), B, H8, W8), groups), B, H8, W8, groups, rec.path, rec.image))
            return orig(lib, descs, B, H8, W8, like)

        self._cls.conv2d = conv2d
        return self

    def __exit__(self, *exc):
        self._cls.conv2d = self._orig
        return False


# ---------------------------------------------------------------------------------------------------------------------
# case builder
# ---------------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    launch: Launch
    B: int
    H: int
    W: int
    descs: list
    groups: List[dict]                 # per group: layout + tensors
    keep: list = field(default_factory=list)


def _cpc(prec):
    return 64 if prec == 2 else 32


def _out_cols(g) -> Dict[str, List[tuple]]:
    """Columns [a, b) of `out` / `aux_out` a launch writes (aux columns relative to the aux row)."""
    epi, cout = g["epilogue"], g["cout"]
    if epi in (2, 4):
        out = [(g["off_out"], g["off_out"] + 128)]
    else:
        out = [(g["off_out"], g["off_out"] + cout)]
    aux = []
    if epi == 2:
        aux = [(0, 128)] + ([(128, 256)] if g["save_gates"] else [])
    elif epi == 4:
        aux = [(0, 128)]
    elif epi == 3 and g["save_gates"]:
        aux = [(0, 128)]
    return {"out": out, "aux": aux}


def _twin_from(x_rows: torch.Tensor) -> torch.Tensor:
    """fp32 [rows, 32 n] -> bf16 split twin [rows, n, 2, 32] (hi = bf16(x) RNE, lo = bf16(x - hi))."""
    hi = x_rows.to(torch.bfloat16)
    lo = (x_rows - hi.float()).to(torch.bfloat16)
    shp = (x_rows.shape[0], x_rows.shape[1] // 32, 1, 32)
    return torch.cat([hi.reshape(shp), lo.reshape(shp)], 2).contiguous()


def _operand_form(x_rows, lds, prec, off, c, gen):
    """Twin / f16 map of an input segment whose live columns [off, off + c) hold x_rows; other whole columns hold noise and
    the columns past off + c up to the end of its chunk are zero (the contract of the all-DMA kernel)."""
    cpc = _cpc(prec)
    rows, width = x_rows.shape[0], lds * cpc
    full = (torch.randn(rows, width, generator=gen) * 50).to(x_rows.device)
    full[:, off:off + c] = x_rows
    end = min(width, (off + c + cpc - 1) // cpc * cpc)
    full[:, off + c:end] = 0
    return full.half().contiguous() if prec == 2 else _twin_from(full)


def _sentinel_form(rows, lds, prec, device, zero_from=None, zero_to=None):
    """Output twin / f16 map full of the sentinel, columns [zero_from, zero_to) zero (the tail of a partial last chunk)."""
    if prec == 2:
        t = torch.full((rows, lds * 64), SENT_BF16, dtype=torch.float16, device=device)
        if zero_from is not None:
            t[:, zero_from:zero_to] = 0
        return t
    t = torch.full((rows, lds, 2, 32), SENT_BF16, dtype=torch.bfloat16, device=device)
    if zero_from is not None and zero_to > zero_from:
        t[:, zero_from // 32, :, zero_from % 32:(zero_to - 1) % 32 + 1] = 0
    return t


def _rand_inputs(gen, rows, c, device):
    x = torch.randn(rows, c, generator=gen)
    x[torch.rand(rows, c, generator=gen) < 0.1] = 0.0                 # exact zeros
    return x.to(device)


def build_case(lib, launch: Launch, B: int, H: int, W: int, device, seed: int = 0) -> Case:
    """Fresh buffers with the recorded layout of `launch` at geometry (B, H, W), seeded data, descriptors for lib.conv2d."""
    from prior_flow_amd import _lib
    from prior_flow_amd.engine import _zero_block
    gen = torch.Generator().manual_seed(seed)
    descs, groups = [], []
    for gi, lay in enumerate(launch.groups):
        g = dict(lay)
        prec, s = g["precision"], g["stride"]
        kh, kw, cout = g["kh"], g["kw"], g["cout"]
        cin = g["c0"] + g["c1"]
        rows_in, rows = B * H * s * W * s, B * H * W
        T = {}
        # weights / bias: scale 1/sqrt(fan_in); packed like the engine does it
        w = torch.randn(cout, cin, kh, kw, generator=gen) / math.sqrt(cin * kh * kw)
        b = (torch.rand(cout, generator=gen) - 0.5)
        from prior_flow_amd.engine import Conv, pack_mfma
        wp, bp = pack_mfma(w.to(device), b.to(device))
        cv = Conv(wp, bp, kh, kw, cin, cout, prec)
        T["w"], T["b"], T["conv"] = w.to(device), b.to(device), cv
        d = _lib.ConvDesc()
        for k in INT_FIELDS:
            setattr(d, k, g[k])
        d.scale = g["scale"]
        d.weight, d.bias = cv.w.data_ptr(), cv.b.data_ptr()
        # input segments
        segs = [("0", g["c0"], g["off0"], g["ld0"], g["lds0"])] + ([("1", g["c1"], g["off1"], g["ld1"], g["lds1"])] if g["c1"] > 0 else [])
        xs = []
        for tag, c, off, ld, lds in segs:
            x = _rand_inputs(gen, rows_in, c, device)
            xs.append(x)
            if g["has_in" + tag]:
                buf = torch.full((rows_in, ld), SENT_IN, device=device)
                buf[:, off:off + c] = x
                T["in" + tag] = buf
                setattr(d, "in" + tag, buf.data_ptr())
            if g["has_in%s_split" % tag]:
                t = _operand_form(x, lds, prec, off, c, gen)
                T["in%s_split" % tag] = t
                setattr(d, "in%s_split" % tag, t.data_ptr())
        T["x"] = torch.cat(xs, 1)                                       # [rows_in, cin] the virtual concatenation
        if g["has_zeros"]:
            zb = _zero_block(device)
            T["zeros"] = zb
            d.zeros, d.zeros_bytes = zb.data_ptr(), zb.numel() * 4
        if g["has_in_scale"]:
            T["in_scale"] = (torch.rand(B, cin, generator=gen) + 0.5).to(device)
            T["in_shift"] = (torch.rand(B, cin, generator=gen) - 0.5).to(device)
            d.in_scale, d.in_shift = T["in_scale"].data_ptr(), T["in_shift"].data_ptr()
        # outputs (sentinel outside the written columns); h may alias out
        cols = _out_cols(g)
        if g["has_out"]:
            T["out"] = torch.full((rows, g["ld_out"]), SENT_F32, device=device)
            d.out = T["out"].data_ptr()
        if g["has_out_split"]:
            a, e = cols["out"][0]
            T["out_split"] = _sentinel_form(rows, g["lds_out"], prec, device, e, min(g["lds_out"] * _cpc(prec), (e + _cpc(prec) - 1) // _cpc(prec) * _cpc(prec)))
            d.out_split = T["out_split"].data_ptr()
        if g["has_aux_out"]:
            T["aux_out"] = torch.full((rows, g["ld_aux"]), SENT_F32, device=device)
            d.aux_out = T["aux_out"].data_ptr()
        if g["has_aux_split"]:
            T["aux_split"] = _sentinel_form(rows, g["lds_aux"], prec, device)
            d.aux_split = T["aux_split"].data_ptr()
        if g["has_h"]:
            hv = torch.randn(rows, g["cout"] if g["epilogue"] != 2 else 128, generator=gen)
            if g["epilogue"] == 6:                                       # the ReLU mask: half <= 0, exact +0.0 and -0.0 among them
                hv = hv.abs() * torch.where(torch.rand(hv.shape, generator=gen) < 0.5, -1.0, 1.0)
                pick = torch.rand(hv.shape, generator=gen)
                hv[pick < 0.08] = 0.0
                hv[pick > 0.92] = -0.0
            hv = hv.to(device)
            T["h_val"] = hv
            if g["alias_h"]:
                T["out"][:, g["off_out"]:g["off_out"] + hv.shape[1]] = hv
                d.h, d.ld_h = T["out"].data_ptr() + 4 * g["off_out"], g["ld_out"]
            else:
                T["h"] = torch.full((rows, g["ld_h"]), SENT_IN, device=device)
                T["h"][:, :hv.shape[1]] = hv
                d.h = T["h"].data_ptr()
        if g["has_z"]:
            zv = torch.rand(rows, g["cout"], generator=gen).to(device)
            T["z_val"] = zv
            T["z"] = torch.full((rows, g["ld_z"]), SENT_IN, device=device)
            T["z"][:, :zv.shape[1]] = zv
            d.z = T["z"].data_ptr()
        if g["has_pre"]:
            pv = (torch.randn(rows, cout, generator=gen) * 0.5).to(device)
            T["pre_val"] = pv
            T["pre"] = torch.full((rows, g["ld_pre"]), SENT_IN, device=device)
            T["pre"][:, g["off_pre"]:g["off_pre"] + cout] = pv
            d.pre = T["pre"].data_ptr()
        g["T"] = T
        descs.append(d)
        groups.append(g)
    if any(g["has_stats_out"] for g in groups):
        nblk = int(lib.conv2d_stats_blocks(descs, B, H, W))
        for g, d in zip(groups, descs):
            if g["has_stats_out"]:
                st = torch.full((B, nblk, g["cout"], 2), float("nan"), dtype=torch.float64, device=device)
                g["T"]["stats"], g["nblk"] = st, nblk
                d.stats_out = st.data_ptr()
    return Case(launch, B, H, W, descs, groups)


def run_case(lib, case: Case):
    like = next(t for t in case.groups[0]["T"].values() if isinstance(t, torch.Tensor) and t.is_cuda)
    lib.conv2d(case.descs, case.B, case.H, case.W, like)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# float64 reference
# ---------------------------------------------------------------------------------------------------------------------
def conv_fp64(x, w, B, H, W, stride, terms=("acc", "abs", "sq"), max_elems=1 << 27):
    """x [B*Hin*Win, cin] channel-last, w [cout, cin, kh, kw]: the convolution (odd k: window [-k/2, k/2]; even k:
    [-k/2, k/2 - 1]) in float64, one float64 matmul per tap (an unfold split by taps), in chunks of images.  Returns
    {"acc": sum x w, "abs": sum |x w|, "sq": sum (x w)^2} as [B*H*W, cout] float64."""
    cout, cin, kh, kw = w.shape
    Hin, Win = H * stride, W * stride
    x = x.reshape(B, Hin, Win, cin)
    wt = w.double().permute(2, 3, 1, 0).reshape(kh * kw, cin, cout)
    out = {t: torch.zeros(B, H, W, cout, dtype=torch.float64, device=x.device) for t in terms}
    per = max(1, max_elems // max(1, (Hin + kh) * (Win + kw) * cin))
    pt, pl = kh // 2, kw // 2
    for b0 in range(0, B, per):
        xb = x[b0:b0 + per].double()
        xp = torch.nn.functional.pad(xb, (0, 0, pl, kw - 1 - pl + stride, pt, kh - 1 - pt + stride))
        nb = xb.shape[0]
        for ky in range(kh):
            for kx in range(kw):
                xs = xp[:, ky:ky + stride * H:stride, kx:kx + stride * W:stride, :].reshape(-1, cin)
                wk = wt[ky * kw + kx]
                if "acc" in terms:
                    out["acc"][b0:b0 + nb] += (xs @ wk).view(nb, H, W, cout)
                if "abs" in terms:
                    out["abs"][b0:b0 + nb] += (xs.abs() @ wk.abs()).view(nb, H, W, cout)
                if "sq" in terms:
                    out["sq"][b0:b0 + nb] += ((xs * xs) @ (wk * wk)).view(nb, H, W, cout)
    return {t: v.view(B * H * W, cout) for t, v in out.items()}


def effective_input(g, B, H, W):
    """The operand the launch convolves, float64: fp32 values (fp16-rounded for PF_PREC_F16), after relu?(x s + t)."""
    T = g["T"]
    x = T["x"]
    s = g["stride"]
    if g["precision"] == 2:
        x = x.half()
    x = x.double()
    if g["has_in_scale"]:
        rows_img = H * s * W * s
        x = x.view(B, rows_img, -1) * T["in_scale"].double()[:, None, :] + T["in_shift"].double()[:, None, :]
        if g["in_relu"]:
            x = x.clamp_min(0)
        x = x.reshape(B * rows_img, -1)
    return x


def reference(case: Case, conv=None) -> List[Dict[str, dict]]:
    """Per group: {output name: {"ref", "tol_elem", "tol_agg", "R"}} in float64.  `conv`: an override of conv_fp64 (the
    CPU teeth test feeds emulated kernels through the same bounds)."""
    res = []
    for g in case.groups:
        T = g["T"]
        prec = g["precision"]
        w = T["w"].half() if prec == 2 else T["w"]
        x = effective_input(g, case.B, case.H, case.W)
        r = (conv or conv_fp64)(x, w.double(), case.B, case.H, case.W, g["stride"])
        K = g["kh"] * g["kw"] * (g["c0"] + g["c1"])
        b = T["b"].double()[None, :]
        v = r["acc"] + b
        A = r["abs"] + b.abs()
        R2 = r["sq"] + b * b
        if g["has_pre"]:
            p = T["pre_val"].double()
            v, A, R2 = v + p, A + p.abs(), R2 + p * p
        R = R2.sqrt()
        eE, eA = C_ELEM * _u_elem(prec, K) * A, K_AGG * _u_agg(prec, K) * R
        res.append(_epilogue(g, v, eE, eA, R))
    return res


def _epilogue(g, v, eE, eA, R):
    """Outputs of the epilogue and both error bounds carried through it (module docstring)."""
    T, epi, sc = g["T"], g["epilogue"], g["scale"]
    h = T["h_val"].double() if "h_val" in T else None
    z = T["z_val"].double() if "z_val" in T else None
    out = {}

    def put(name, ref, lipE, lipA, tail, Reff):
        out[name] = {"ref": ref, "tol_elem": lipE + tail, "tol_agg": lipA + tail, "tail": tail + 0 * ref, "R": Reff}

    if epi == 0:
        put("out", v * sc, abs(sc) * eE, abs(sc) * eA, EPS_EPI * (v * sc).abs(), abs(sc) * R)
    elif epi == 1:
        put("out", v.clamp_min(0), eE, eA, EPS_EPI * v.abs(), R)
    elif epi == 2:
        zz = torch.sigmoid(v[:, :128])
        put("out", zz, eE[:, :128], eA[:, :128], EPS_TRANS + 0 * zz, R[:, :128])
        rr = torch.sigmoid(v[:, 128:])
        ah = h.abs()
        aux = {"rh": (rr * h, ah * eE[:, 128:], ah * eA[:, 128:], ah * EPS_TRANS + EPS_EPI * ah, ah * R[:, 128:])}
        if g["save_gates"]:
            aux["r"] = (rr, eE[:, 128:], eA[:, 128:], EPS_TRANS + 0 * rr, R[:, 128:])
        out["aux_parts"] = aux
    elif epi == 3:
        q = torch.tanh(v)
        o = (1 - z) * h + z * q
        put("out", o, z * eE, z * eA, z * EPS_TRANS + EPS_EPI * (h.abs() + q.abs()), z * R)
        if g["save_gates"]:
            out["aux_parts"] = {"q": (q, eE, eA, EPS_TRANS + 0 * q, R)}
    elif epi == 4:
        put("out", torch.tanh(v[:, :128]), eE[:, :128], eA[:, :128], EPS_TRANS + 0 * v[:, :128], R[:, :128])
        out["aux_parts"] = {"inp": (v[:, 128:].clamp_min(0), eE[:, 128:], eA[:, 128:], EPS_EPI * v[:, 128:].abs(), R[:, 128:])}
    elif epi == 5:
        o = (h + v.clamp_min(0)).clamp_min(0)
        put("out", o, eE, eA, EPS_EPI * (h.abs() + v.abs()), R)
    elif epi == 6:
        m = (h > 0).double()
        put("out", m * v * sc, m * abs(sc) * eE, m * abs(sc) * eA, m * EPS_EPI * (v * sc).abs(), m * abs(sc) * R)
    elif epi == 7:
        put("out", v * sc + h, abs(sc) * eE, abs(sc) * eA, EPS_EPI * ((v * sc).abs() + h.abs()), abs(sc) * R)
    if "aux_parts" in out:          # aux columns: [0, 128) r*h / q / inp, [128, 256) r
        parts = out.pop("aux_parts")
        first = parts.get("rh") or parts.get("q") or parts.get("inp")
        cols = [first] + ([parts["r"]] if "r" in parts else [])
        cat = lambda i: torch.cat([c[i] for c in cols], 1)             # noqa: E731
        out["aux"] = {"ref": cat(0), "tol_elem": cat(1) + cat(3), "tol_agg": cat(2) + cat(3), "tail": cat(3), "R": cat(4)}
    return out


# ---------------------------------------------------------------------------------------------------------------------
# checks
# ---------------------------------------------------------------------------------------------------------------------
def _twin_values(t: torch.Tensor) -> torch.Tensor:
    return (t[:, :, 0, :].double() + t[:, :, 1, :].double()).reshape(t.shape[0], -1)


def compare(got, r, what, fails, rep_err=None):
    """got vs reference r (float64 [rows, w]) under both bounds; appends messages to `fails`.  Returns the worst
    (|err| / per-element bound, (|err| - epilogue tail) / aggregate bound): both <= 1 when the checks pass."""
    err = (got.double() - r["ref"]).abs()
    err = torch.where(torch.isnan(got.double()), torch.full_like(err, float("inf")), err)
    extra = rep_err if rep_err is not None else torch.zeros_like(err)
    te, ta = r["tol_elem"] + extra, r["tol_agg"] + extra
    be, ba = err > te, err > ta
    if not err.numel():
        return 0.0, 0.0
    ratio_e = float((err / te.clamp_min(1e-300)).max())
    lin = (r["tol_agg"] - r["tail"]).clamp_min(1e-300)
    ratio_a = float(((err - r["tail"] - extra).clamp_min(0) / lin).max())
    for bad, kind, tol in ((be, "per-element", te), (ba, "aggregate", ta)):
        if bool(bad.any()):
            i = tuple(int(v) for v in torch.nonzero(bad)[0])
            fails.append(f"{what}: {int(bad.sum())} elements beyond the {kind} bound (worst err/bound {ratio_e if kind == 'per-element' else ratio_a:.3g}), "
                         f"first at row {i[0]} col {i[1]}: got {float(got[i]):.7g} want {float(r['ref'][i]):.7g} bound {float(tol[i]):.3g}")
    return ratio_e, ratio_a


def _is_split(hi, lo) -> bool:
    """hi = bf16(v), lo = bf16(v - hi) for some v: |lo| <= half an ulp of hi (lo == 0 where hi == 0)."""
    bits = hi.view(torch.int16).to(torch.int32) & 0x7FFF
    mag = bits.to(torch.int16).view(torch.bfloat16).float()
    nxt = (bits + 1).to(torch.int16).view(torch.bfloat16).float()
    ok = torch.where(bits == 0, lo.float() == 0, lo.float().abs() <= 0.5 * (nxt - mag))
    return bool(ok.all())


def _check_twin(twin, vals32, cols, prec, what, fails, zero_tail):
    """Output twin / map: written columns == split / .half() of the fp32 output bit for bit (vals32 None: a consistent hi|lo
    split), the zero tail past the written columns still zero, every other column still the sentinel."""
    rows = twin.shape[0]
    cpc = _cpc(prec)
    width = twin.numel() // rows // (1 if prec == 2 else 2)
    written = torch.zeros(width, dtype=torch.bool, device=twin.device)
    zero = torch.zeros(width, dtype=torch.bool, device=twin.device)
    for a, e in cols:
        written[a:e] = True
    if zero_tail:
        zero[zero_tail[0]:zero_tail[1]] = True
    if prec == 2:
        flat = twin.view(rows, width)
        for (a, e), v in zip(cols, vals32 or [None] * len(cols)):
            if v is not None and not torch.equal(flat[:, a:e], v.half()):
                fails.append(f"{what}: f16 map columns [{a},{e}) differ from .half() of the fp32 output")
        rest = flat[:, ~written & ~zero]
        if not bool((rest == SENT_BF16).all()) or not bool((flat[:, zero] == 0).all()):
            fails.append(f"{what}: f16 map written outside its columns (or its zero tail)")
        return
    hi = twin.view(rows, width // cpc, 2, cpc)[:, :, 0, :].reshape(rows, width)
    lo = twin.view(rows, width // cpc, 2, cpc)[:, :, 1, :].reshape(rows, width)
    for (a, e), v in zip(cols, vals32 or [None] * len(cols)):
        if v is not None:
            vh = v.to(torch.bfloat16)
            vl = (v - vh.float()).to(torch.bfloat16)
            if not (torch.equal(hi[:, a:e], vh) and torch.equal(lo[:, a:e], vl)):
                fails.append(f"{what}: twin columns [{a},{e}) differ from split_bf16 of the fp32 output")
        elif not _is_split(hi[:, a:e], lo[:, a:e]):
            fails.append(f"{what}: twin columns [{a},{e}) are no hi|lo split (|lo| > half an ulp of hi)")
    keep = ~written & ~zero
    if not (bool((hi[:, keep] == SENT_BF16).all()) and bool((lo[:, keep] == SENT_BF16).all())
            and bool((hi[:, zero] == 0).all()) and bool((lo[:, zero] == 0).all())):
        fails.append(f"{what}: twin written outside its columns (or its zero tail)")


def check_case(case: Case, refs) -> (List[str], dict):
    """All checks of one run case; returns (failures, worst ratios {"elem": .., "agg": ..})."""
    fails, worst = [], {"elem": 0.0, "agg": 0.0}
    for gi, (g, ref) in enumerate(zip(case.groups, refs)):
        T, prec = g["T"], g["precision"]
        cols = _out_cols(g)
        for name in ("out", "aux"):
            if name not in ref:
                continue
            f32_key, split_key = ("out", "out_split") if name == "out" else ("aux_out", "aux_split")
            c = cols[name]
            r = ref[name]
            what = f"group {gi} {name}"
            got32 = None
            if g["has_" + f32_key]:
                buf = T[f32_key]
                got32 = torch.cat([buf[:, a:e] for a, e in c], 1)
                ratios = compare(got32, r, what, fails)
                worst = {"elem": max(worst["elem"], ratios[0]), "agg": max(worst["agg"], ratios[1])}
                # sentinels: everything outside the written columns (the aliased h columns were overwritten on purpose)
                mask = torch.ones(buf.shape[1], dtype=torch.bool, device=buf.device)
                for a, e in c:
                    mask[a:e] = False
                if not bool((buf[:, mask] == SENT_F32).all()):
                    fails.append(f"{what}: fp32 buffer written outside columns {c}")
            if g["has_" + split_key]:
                tw = T[split_key]
                if name == "aux":          # the twin of aux holds r*h / q / inp only, never the saved r gate
                    c = c[:1]
                    r = {k: v[:, :128] for k, v in r.items()}
                vals = [buf[:, a:e] for a, e in c] if got32 is not None else None
                end = c[-1][1]
                cpc = _cpc(prec)
                width = g["lds_out" if name == "out" else "lds_aux"] * cpc
                tail = (end, min(width, (end + cpc - 1) // cpc * cpc)) if name == "out" else None
                _check_twin(tw, vals, c, prec, what + " " + ("f16 map" if prec == 2 else "twin"), fails, tail)
                if got32 is None:         # twin only: its values against the reference, plus their representation error
                    if prec == 2:
                        v = torch.cat([tw.view(tw.shape[0], -1)[:, a:e] for a, e in c], 1).double()
                        rep = (r["ref"].abs() + r["tol_elem"]) * 2.0 ** -11 + 2.0 ** -25
                    else:
                        full = _twin_values(tw)
                        v = torch.cat([full[:, a:e] for a, e in c], 1)
                        rep = (r["ref"].abs() + r["tol_elem"]) * 2.0 ** -16
                    ratios = compare(v, r, what + " (twin values)", fails, rep)
                    worst = {"elem": max(worst["elem"], ratios[0]), "agg": max(worst["agg"], ratios[1])}
        if g["has_stats_out"]:
            st = T["stats"]
            if g["has_out"]:
                y = T["out"][:, g["off_out"]:g["off_out"] + g["cout"]].double()
            else:
                y = _twin_values(T["out_split"])[:, g["off_out"]:g["off_out"] + g["cout"]]
            y = y.view(case.B, -1, g["cout"])
            if not bool(torch.isfinite(st).all()):
                fails.append(f"group {gi} stats: {int((~torch.isfinite(st)).sum())} partials never written")
            s1, s2 = st[..., 0].sum(1), st[..., 1].sum(1)
            w1, w2 = y.sum(1), (y * y).sum(1)
            tol1 = 1e-9 * y.abs().sum(1) + 1e-12
            if bool(((s1 - w1).abs() > tol1).any()) or bool(((s2 - w2).abs() > 1e-9 * w2 + 1e-12).any()):
                fails.append(f"group {gi} stats: partial sums differ from fp64 sums of the output "
                             f"(max {float((s1 - w1).abs().max()):.3g} / {float((s2 - w2).abs().max()):.3g})")
    return fails, worst


# ---------------------------------------------------------------------------------------------------------------------
# geometry
# ---------------------------------------------------------------------------------------------------------------------
def fake_descs(launch: Launch):
    """Descriptors with the recorded layout and placeholder pointers: enough for the host planners, never launched."""
    from prior_flow_amd import _lib
    out = []
    for g in launch.groups:
        d = _lib.ConvDesc()
        for k in INT_FIELDS:
            setattr(d, k, g[k])
        d.scale = g["scale"]
        base = 0x100000
        for i, k in enumerate(PTR_FIELDS):
            if g["has_" + k]:
                setattr(d, k, base + 0x10000000 * (i + 1))
        if g["alias_h"]:
            d.h = d.out + 4 * g["off_out"]
        out.append(d)
    return out


def same_signature(lib, launch: Launch, B, H, W) -> bool:
    descs = fake_descs(launch)
    try:
        tr = plan(lib, descs, B, H, W)
    except Exception:
        return False
    if tr[0] < 0 or tr[1] < 0:
        return False
    if any(g["has_stats_out"] for g in launch.groups) and int(lib._dll.pf_conv2d_stats_blocks(
            (type(descs[0]) * len(descs))(*descs), len(descs), B, H, W)) <= 0:
        return False
    return signature_of_layouts(tr, launch.groups) == launch.sig


def ragged_sibling(lib, launch: Launch):
    """A geometry near the launch's with the same signature and B >= 2, H odd (no multiple of any tile height), W odd (no
    multiple of 32; B*H*W then no multiple of any generic tile's BM either), or None.  Candidates are scored by how far
    their pixel count is from the product's."""
    B, H, W = launch.B, launch.H, launch.W
    target = B * H * W
    best = None
    fac = (1.0, 0.75, 0.5, 1.25, 0.35, 0.25, 1.5, 0.18, 0.12, 2.0)
    for Bc in sorted({2, 3, max(2, B), max(2, B // 2), max(2, B // 4), B + 1}):
        for fh in fac:
            for fw in fac:
                Hc = max(3, int(H * fh)) | 1
                Wc = max(3, int(W * fw)) | 1
                if not same_signature(lib, launch, Bc, Hc, Wc):
                    continue
                score = abs(math.log(Bc * Hc * Wc / target))
                if best is None or score < best[0]:
                    best = (score, (Bc, Hc, Wc))
    return None if best is None else best[1]


def why_no_sibling(lib, launch: Launch) -> str:
    """A plain reason when ragged_sibling finds nothing."""
    t = launch.sig[3]
    if t == "tile6":
        return "tile 6 (weights-stationary encoder kernel) needs whole 32-column strips: W % 32 == 0"
    if any(g["has_stats_out"] for g in launch.groups) and launch.sig[3] in ("tile0", "tile1", "tile2", "tile7"):
        return "fused statistics on the generic kernel need H*W % BM == 0"
    return "no candidate near the product geometry keeps the signature (tile / roles choice depends on the work-item count)"


# ---------------------------------------------------------------------------------------------------------------------
# the plans a layout reaches
# ---------------------------------------------------------------------------------------------------------------------
# Image geometries the product is run at by a test, the bench or DESIGN.md (1920x3840: the panorama of section 10); a
# bidirectional stream doubles B, which the batches below cover.
GRID_SIZES = ((128, 256), (136, 216), (160, 360), (256, 512), (384, 512), (480, 960), (512, 1024), (640, 1280), (1024, 2048),
              (1920, 3840))
GRID_BATCHES = (1, 2, 3, 4, 8, 16, 32)
GRID = tuple((B, H, W) for H, W in GRID_SIZES for B in GRID_BATCHES)


def relation(launch: Launch):
    """(m, d) of a recorded launch: m = launch.B / B_img images per pair the layer sees (2 frames, 4 with the rotated
    ones, ...), d = H_img / launch.H = W_img / launch.W the layer's resolution divisor.  Both are positive integers in
    every layer of the model; anything else is an error that names the launch."""
    if not launch.image:
        raise ValueError(f"launch without the image geometry of its path: {sig_str(launch.sig)}")
    Bi, Hi, Wi = launch.image
    ok = min(Bi, Hi, Wi, launch.B, launch.H, launch.W) > 0 and launch.B % Bi == 0 and Hi % launch.H == 0 and \
        Wi % launch.W == 0 and Hi // launch.H == Wi // launch.W
    if not ok:
        raise ValueError(f"launch {launch.B}x{launch.H}x{launch.W} in a path of {Bi}x{Hi}x{Wi} images is no whole number of "
                         f"images per pair at a whole resolution divisor: {sig_str(launch.sig)}")
    return launch.B // Bi, Hi // launch.H


def _desc_array(descs):
    return (type(descs[0]) * len(descs))(*descs)


def reachable(lib, launch: Launch, grid=GRID) -> Dict[tuple, List[tuple]]:
    """{signature: [launch geometry (B, H, W), ...]} of every plan the planner gives the layout of `launch` over the image
    geometries of `grid`: an image geometry (B, H, W) is the launch geometry (m B, H / d, W / d) with relation(launch)'s
    (m, d); sizes d does not divide, geometries the planner refuses and launches with stats_out the planner gives no
    statistics blocks (the rule of same_signature) are left out.  The launch's own signature is among the keys when the
    grid holds its image geometry.

    The layout is held fixed while the geometry moves.  That over-approximates what the product reaches: the engine may
    build another layout at another size (fp32 rows instead of twins, a separate statistics pass, another co_groups), so a
    signature found here need not be one the product launches.  A plan the product never takes costs its replay a few
    seconds; a plan it takes that nobody checked costs a wrong flow."""
    m, d = relation(launch)
    descs = fake_descs(launch)
    arr = _desc_array(descs)
    stats = any(g["has_stats_out"] for g in launch.groups)
    out: Dict[tuple, List[tuple]] = {}
    for Bi, Hi, Wi in grid:
        if Hi % d or Wi % d:
            continue
        geo = (m * Bi, Hi // d, Wi // d)
        tr = plan(lib, descs, *geo)
        if tr[0] < 0 or tr[1] < 0:
            continue
        if stats and int(lib._dll.pf_conv2d_stats_blocks(arr, len(descs), *geo)) <= 0:
            continue
        geos = out.setdefault(signature_of_layouts(tr, launch.groups), [])
        if geo not in geos:
            geos.append(geo)
    return out


def with_signature(launch: Launch, sig, B, H, W) -> Launch:
    """The launch's layout under another plan and geometry (what same_signature and ragged_sibling compare against)."""
    return Launch(sig, B, H, W, launch.groups, launch.path, launch.image)


def witness(lib, launch: Launch, sig, geos, ragged: bool = True):
    """The geometry at which to replay signature `sig` of the layout of `launch`, out of reachable()'s `geos`:
    (B, H, W, was_made_ragged).  The candidate with the fewest output pixels x groups (ties: H odd or W no multiple of 32
    first), then -- unless `ragged` is False -- its ragged sibling (B >= 2, H and W odd, near the candidate's size) where
    the planner keeps the signature there."""
    ng = len(launch.groups)
    B, H, W = min(geos, key=lambda g: (g[0] * g[1] * g[2] * ng, 0 if (g[1] % 2 or g[2] % 32) else 1, g))
    if ragged:
        probe = with_signature(launch, sig, B, H, W)
        sib = ragged_sibling(lib, probe)
        if sib is not None and same_signature(lib, probe, *sib):
            return sib + (True,)
    return B, H, W, False
