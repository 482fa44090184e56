"""Every weight-gradient launch the product makes, replayed against a float64 reference (helper of
test_hip_wgrad_launches.py, test_wgrad_launch_reference.py and the directed cases of test_hip_conv_bwd.py; not a conftest).

  Recorder                            context manager around PfLib.conv2d_wgrad and PfLib.conv2d_wgrad_small (the Python entries
                                      to pf_conv2d_wgrad / pf_conv2d_wgrad_small[_ws]): per launch every integer argument, each
                                      tensor's leading dimension, dw.shape, whether db and x1 are given, nchw and B, H, W.  That
                                      plain tuple is the signature: there is no planner to query.
  build_case(launch, B, H, W, device) fresh seeded buffers with the recorded layout: SENT_IN in the columns of x0 / x1 / dy
                                      outside the read slices, zeros in the live region of dw / db, a seeded non-zero fp32 pattern
                                      in the padding rows (>= cout) and columns (>= c0 + c1) of dw and in db[cout:].
  run_case(lib, case)                 one launch into the case's buffers (dw, db accumulate: call it twice for 2x).
  reference(case)                     dw and db in float64 with A = sum |terms| and R = sqrt(sum terms^2) per element.
  check_case(case, ref, mult)         both bounds on dw and db against mult x the reference, the padding pattern bit for bit,
                                      the sentinels; returns (failures, worst ratios).

THE OPERATION.  K = B*H*W pixels p (output pixels for the small kernel), zero padding inside each image:
    MFMA kernel    dw[o][tap][c]    = sum_p dy[p][o] * x[p + off(tap)][c]           dw [Cout_pad][kh*kw][Cin_pad32]
    small kernel   dw[o][c][ky][kx] = sum_p dy[p][o] * x[stride*p + (ky,kx) - pad][c]
    both           db[o]            = sum_p dy[p][o]
The reference is one float64 matmul per tap (dy^T @ shifted x), chunked by images, on the device of the operands.

TOLERANCES (the two bounds and the constants C_ELEM, K_AGG of conv_launches.TOLERANCES; here the reduction runs over the K
pixels).  For one element v = sum_p t_p let A = sum_p |t_p| and R = sqrt(sum_p t_p^2).
  * per element,  |err| <= C_ELEM * (U + K * 2^-24) * A
  * aggregate,    max |err| / R <= K_AGG * (U + sqrt(K) * 2^-23)
U is the error of one product relative to |t_p|:
  * MFMA kernel, U = 2^-16: both operands are split into bf16 hi + lo on their way into LDS and the kernel multiplies
    lo*hi + hi*lo + hi*hi; it drops lo*lo (<= 2^-16 |t_p|: each lo is <= 2^-8 of its value) and the rounding of each lo
    (2^-16 of its operand, two operands, but then 2^-17 each: bf16 keeps 8 significant bits) -- as in the forward.
  * small kernel, U = 2^-24: one fp32 fma per product.
  * db, U = 0: a sum of fp32 values.
The K term is the accumulation.  Order of operations of the MFMA kernel: a wave's 32x32 accumulator takes, per 16-pixel step and
pass, an exact-product dot of 16 terms added in fp32 (at most one rounding per term), over all the tiles of its split; then ONE
fp32 atomic per split into dw, in arbitrary order (<= 512 splits).  Every partial sum is a sum of a subset of the t_p, so each
rounding is at most 2^-24 of a value <= A: at most K + nsplit <= 2 K roundings (C_ELEM = 4 absorbs the factor) in the worst
case; their signs are random, so in aggregate they walk: sqrt(K) steps of 2^-24 of a partial sum whose scale is R (the inputs
of build_case are zero-mean, so partial sums are of R's scale and not of A's).  The small kernel has the same shape: fp32 fma
chains per workgroup over its tiles, then per-slice sums and 8 atomics (or one atomic per workgroup).  db: per-thread sums of 8
pixels, LDS atomics per tile, one global atomic per workgroup.
A lost 4x32 pixel tile moves an element by 128 terms, |err| ~ sqrt(128 / K) R: 2^-4 R at K = 36864, against an aggregate bound
of 8 * (2^-16 + 192 * 2^-23) = 3e-4; the per-element bound (K * 2^-24 * A, with A ~ sqrt(K) R) does NOT see it at large K, which
is why both are asserted (test_wgrad_launch_reference.py proves which one catches what).  A lost hi*lo pass errs by ~2^-9 R.
A second launch into the same buffers must give 2x the reference under 2x the bounds (dw and db accumulate).
"""
from __future__ import annotations

import contextlib
import math
from dataclasses import dataclass, field
from typing import List

import torch

from conv_launches import C_ELEM, K_AGG, SENT_IN

U_MFMA, U_SMALL, U_SUM = 2.0 ** -16, 2.0 ** -24, 0.0
TH, TW = 4, 32                       # pixel tile of pf_conv2d_wgrad
WS_T = 8                             # output-pixel tile of pf_conv2d_wgrad_small

MFMA_FIELDS = ("ld0", "off0", "c0", "ld1", "off1", "c1", "ld_dy", "off_dy", "cout", "kh", "kw", "dw_shape", "db_len", "has_x1")
SMALL_FIELDS = ("nchw", "ld_in", "off_in", "cin", "ld_dy", "off_dy", "cout", "kh", "kw", "stride", "dw_shape", "db_len")


def u_elem(U, K):
    return U + K * 2.0 ** -24


def u_agg(U, K):
    return U + math.sqrt(K) * 2.0 ** -23


# ---------------------------------------------------------------------------------------------------------------------
# recorder
# ---------------------------------------------------------------------------------------------------------------------
@dataclass
class Launch:
    kind: str                          # "mfma" | "small"
    args: dict                         # MFMA_FIELDS / SMALL_FIELDS
    B: int
    H: int                             # output map (the small kernel reads stride*H x stride*W inputs)
    W: int
    path: str = ""

    @property
    def sig(self) -> tuple:
        f = MFMA_FIELDS if self.kind == "mfma" else SMALL_FIELDS
        return (self.kind,) + tuple(self.args[k] for k in f) + (self.B, self.H, self.W)


def sig_str(ln: Launch) -> str:
    a = ln.args
    if ln.kind == "mfma":
        segs = f"x0[{a['off0']}:+{a['c0']}]/{a['ld0']}" + (f" x1[{a['off1']}:+{a['c1']}]/{a['ld1']}" if a["c1"] else "")
        return (f"mfma  {a['kh']}x{a['kw']} {segs} dy[{a['off_dy']}:+{a['cout']}]/{a['ld_dy']} dw{list(a['dw_shape'])}"
                f"{' db' if a['db_len'] else ''}  {ln.B}x{ln.H}x{ln.W}")
    src = "nchw" if a["nchw"] else f"x[{a['off_in']}:+{a['cin']}]/{a['ld_in']}"
    return (f"small {a['kh']}x{a['kw']}/{a['stride']} cin{a['cin']} {src} dy[{a['off_dy']}:+{a['cout']}]/{a['ld_dy']}"
            f"{' db' if a['db_len'] else ''}  {ln.B}x{ln.H}x{ln.W}")


class Recorder(contextlib.AbstractContextManager):
    """Wraps PfLib.conv2d_wgrad and PfLib.conv2d_wgrad_small on the class: every launch is recorded, then runs as before.
    Enter it before the model exists (a bound method cached by it would otherwise escape)."""

    def __init__(self, path: str = ""):
        self.path = path
        self.launches: List[Launch] = []

    def __enter__(self):
        from prior_flow_amd import _lib
        self._cls = _lib.PfLib
        self._orig = (_lib.PfLib.conv2d_wgrad, _lib.PfLib.conv2d_wgrad_small)
        orig_m, orig_s = self._orig
        rec = self

        def conv2d_wgrad(lib, x0, off0, c0, dy, off_dy, cout, dw, db, kh, kw, B, H8, W8, x1=None, off1=0, c1=0):
            a = dict(ld0=int(x0.shape[-1]), off0=int(off0), c0=int(c0), ld1=0 if x1 is None else int(x1.shape[-1]), off1=int(off1),
                     c1=int(c1), ld_dy=int(dy.shape[-1]), off_dy=int(off_dy), cout=int(cout), kh=int(kh), kw=int(kw),
                     dw_shape=tuple(int(v) for v in dw.shape), db_len=0 if db is None else int(db.numel()), has_x1=x1 is not None)
            rec.launches.append(Launch("mfma", a, int(B), int(H8), int(W8), rec.path))
            return orig_m(lib, x0, off0, c0, dy, off_dy, cout, dw, db, kh, kw, B, H8, W8, x1=x1, off1=off1, c1=c1)

        def conv2d_wgrad_small(lib, x, nchw, off_in, cin, dy, off_dy, cout, dw, db, kh, kw, stride, B, Hout, Wout, **kwargs):
            a = dict(nchw=bool(nchw), ld_in=0 if nchw else int(x.shape[-1]), off_in=int(off_in), cin=int(cin), ld_dy=int(dy.shape[-1]),
                     off_dy=int(off_dy), cout=int(cout), kh=int(kh), kw=int(kw), stride=int(stride),
                     dw_shape=tuple(int(v) for v in dw.shape), db_len=0 if db is None else int(db.numel()))
            rec.launches.append(Launch("small", a, int(B), int(Hout), int(Wout), rec.path))
            return orig_s(lib, x, nchw, off_in, cin, dy, off_dy, cout, dw, db, kh, kw, stride, B, Hout, Wout, **kwargs)

        self._cls.conv2d_wgrad = conv2d_wgrad
        self._cls.conv2d_wgrad_small = conv2d_wgrad_small
        return self

    def __exit__(self, *exc):
        self._cls.conv2d_wgrad, self._cls.conv2d_wgrad_small = self._orig
        return False


def mfma_launch(kh, kw, c0, cout, B, H, W, c1=0, off0=0, off1=0, off_dy=0, pad0=0, pad1=0, pad_dy=0, db=True, dw_rows=None,
                path="directed") -> Launch:
    """A launch written by hand (the directed cases): row lengths = offset + channels + pad."""
    rows = dw_rows or (cout + 127) // 128 * 128
    a = dict(ld0=off0 + c0 + pad0, off0=off0, c0=c0, ld1=(off1 + c1 + pad1) if c1 else 0, off1=off1, c1=c1, ld_dy=off_dy + cout + pad_dy,
             off_dy=off_dy, cout=cout, kh=kh, kw=kw, dw_shape=(rows, kh * kw, (c0 + c1 + 31) // 32 * 32), db_len=rows if db else 0,
             has_x1=c1 > 0)
    return Launch("mfma", a, B, H, W, path)


def small_launch(cin, cout, kh, kw, stride, B, Ho, Wo, nchw=True, off_in=0, pad_in=0, off_dy=0, pad_dy=0, db=True,
                 path="directed") -> Launch:
    a = dict(nchw=bool(nchw), ld_in=0 if nchw else off_in + cin + pad_in, off_in=off_in, cin=cin, ld_dy=off_dy + cout + pad_dy,
             off_dy=off_dy, cout=cout, kh=kh, kw=kw, stride=stride, dw_shape=(cout, cin, kh, kw), db_len=cout if db else 0)
    return Launch("small", a, B, Ho, Wo, path)


# ---------------------------------------------------------------------------------------------------------------------
# geometry
# ---------------------------------------------------------------------------------------------------------------------
def tiles(ln: Launch, B=None, H=None, W=None) -> int:
    """Pixel tiles of a launch: 4 x 32 for the MFMA kernel, 8 x 8 output pixels for the small one."""
    B, H, W = ln.B if B is None else B, ln.H if H is None else H, ln.W if W is None else W
    th, tw = (TH, TW) if ln.kind == "mfma" else (WS_T, WS_T)
    return B * ((H + th - 1) // th) * ((W + tw - 1) // tw)


def mfma_splits(ln: Launch, B=None, H=None, W=None) -> int:
    """The split count the header of pf_conv2d_wgrad promises: min(ceil(512 / workgroups), pixel tiles), never above 512."""
    a = ln.args
    cin_pad = (a["c0"] + a["c1"] + 31) // 32 * 32
    wg_c = 32 if a["kh"] * a["kw"] > 5 else 64
    wg = ((a["cout"] + 127) // 128) * ((cin_pad + wg_c - 1) // wg_c)
    return max(1, min((512 + wg - 1) // wg, tiles(ln, B, H, W)))


def ragged_sibling(ln: Launch):
    """(B, H - 1, W - 3) when that keeps the tile count (and with it the splits / the workgroup count): partial tiles on both
    axes; else None."""
    H, W = ln.H - 1, ln.W - 3
    if H < 1 or W < 1 or tiles(ln, ln.B, H, W) != tiles(ln):
        return None
    return ln.B, H, W


# ---------------------------------------------------------------------------------------------------------------------
# case builder
# ---------------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    launch: Launch
    B: int
    H: int
    W: int
    T: dict = field(default_factory=dict)


def _rand(gen, rows, c, device):
    x = torch.randn(rows, c, generator=gen, device=device)
    x[torch.rand(rows, c, generator=gen, device=device) < 0.1] = 0.0    # exact zeros
    return x


def _pattern(gen, shape, device):
    """Seeded fp32 values, none of them zero (|v| in [0.5, 1.5))."""
    v = torch.rand(shape, generator=gen, device=device) + 0.5
    return v * torch.where(torch.rand(shape, generator=gen, device=device) < 0.5, -1.0, 1.0)


def _rows_buf(vals, ld, off, device):
    buf = torch.full((vals.shape[0], ld), SENT_IN, device=device)
    buf[:, off:off + vals.shape[1]] = vals
    return buf


def build_case(launch: Launch, B: int, H: int, W: int, device, seed: int = 0, dy_keep=None) -> Case:
    """Fresh buffers with the recorded layout of `launch` at geometry (B, H, W).  dy_keep: optional [B*H*W] mask of the
    pixels whose output gradient is kept (the others are zero, as in a zero-stuffed stride-2 gradient)."""
    gen = torch.Generator(device=device).manual_seed(seed)      # (values are generated on the device of the case)
    a, T = launch.args, {}
    rows = B * H * W
    dyv = _rand(gen, rows, a["cout"], device)
    if dy_keep is not None:
        dyv = dyv * dy_keep.to(device).view(-1, 1).to(dyv.dtype)
    T["dy_val"], T["dy"] = dyv, _rows_buf(dyv, a["ld_dy"], a["off_dy"], device)
    if launch.kind == "mfma":
        x0 = _rand(gen, rows, a["c0"], device)
        T["x0"] = _rows_buf(x0, a["ld0"], a["off0"], device)
        xs = [x0]
        if a["has_x1"]:
            x1 = _rand(gen, rows, max(a["c1"], 0), device)
            T["x1"] = _rows_buf(x1, a["ld1"], a["off1"], device)
            if a["c1"] > 0:
                xs.append(x1)
        T["x_val"] = torch.cat(xs, 1)
        cin = a["c0"] + a["c1"]
        dw = _pattern(gen, a["dw_shape"], device)
        dw[:a["cout"], :, :cin] = 0
    else:
        s, cin = a["stride"], a["cin"]
        rows_in = B * H * s * W * s
        xv = _rand(gen, rows_in, cin, device)
        T["x_val"] = xv
        if a["nchw"]:
            T["x"] = xv.view(B, H * s, W * s, cin).permute(0, 3, 1, 2).contiguous()
        else:
            T["x"] = _rows_buf(xv, a["ld_in"], a["off_in"], device)
        dw = torch.zeros(a["dw_shape"], device=device)
    T["dw"], T["dw_init"] = dw, dw.clone()
    if a["db_len"]:
        db = _pattern(gen, (a["db_len"],), device)
        db[:a["cout"]] = 0
        T["db"], T["db_init"] = db, db.clone()
    return Case(launch, B, H, W, T)


def run_case(lib, case: Case, **kwargs):
    a, T = case.launch.args, case.T
    if case.launch.kind == "mfma":
        lib.conv2d_wgrad(T["x0"], a["off0"], a["c0"], T["dy"], a["off_dy"], a["cout"], T["dw"], T.get("db"), a["kh"], a["kw"],
                         case.B, case.H, case.W, x1=T.get("x1"), off1=a["off1"], c1=a["c1"])
    else:
        lib.conv2d_wgrad_small(T["x"], a["nchw"], a["off_in"], a["cin"], T["dy"], a["off_dy"], a["cout"], T["dw"], T.get("db"),
                               a["kh"], a["kw"], a["stride"], case.B, case.H, case.W, **kwargs)
    if T["dw"].is_cuda:
        torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# float64 reference
# ---------------------------------------------------------------------------------------------------------------------
def wgrad_fp64(x, dy, B, H, W, kh, kw, stride=1, terms=("acc", "abs", "sq"), max_elems=1 << 25):
    """x [B*(stride H)*(stride W), cin], dy [B*H*W, cout], channel-last: {"acc": sum dy x, "abs": sum |dy x|,
    "sq": sum (dy x)^2} as float64 [cout, kh*kw, cin]; window [-k/2, k - 1 - k/2] around stride * p, zero padding inside
    each image.  One float64 matmul per tap, in chunks of images, on the device of x."""
    cin, cout = x.shape[1], dy.shape[1]
    Hi, Wi = H * stride, W * stride
    x = x.reshape(B, Hi, Wi, cin)
    dy = dy.reshape(B, H * W, cout)
    out = {t: torch.zeros(cout, kh * kw, cin, dtype=torch.float64, device=x.device) for t in terms}
    per = max(1, max_elems // max(1, (Hi + kh) * (Wi + kw) * max(cin, cout)))
    pt, pl = kh // 2, kw // 2
    for b0 in range(0, B, per):
        xp = torch.nn.functional.pad(x[b0:b0 + per].double(), (0, 0, pl, kw - 1 - pl + stride, pt, kh - 1 - pt + stride))
        dt = dy[b0:b0 + per].double().reshape(-1, cout).t()
        for ky in range(kh):
            for kx in range(kw):
                xs = xp[:, ky:ky + stride * H:stride, kx:kx + stride * W:stride, :].reshape(-1, cin)
                tap = ky * kw + kx
                if "acc" in terms:
                    out["acc"][:, tap] += dt @ xs
                if "abs" in terms:
                    out["abs"][:, tap] += dt.abs() @ xs.abs()
                if "sq" in terms:
                    out["sq"][:, tap] += (dt * dt) @ (xs * xs)
    return out


def reference(case: Case) -> dict:
    """{"dw": {"ref", "A", "R", "U"}, "db": {...}, "K"}: dw in the layout of the kernel's dw (live region only)."""
    ln, T = case.launch, case.T
    a = ln.args
    small = ln.kind == "small"
    r = wgrad_fp64(T["x_val"], T["dy_val"], case.B, case.H, case.W, a["kh"], a["kw"], a["stride"] if small else 1)
    if small:          # [cout, taps, cin] -> [Cout][Cin][KH][KW]
        r = {k: v.permute(0, 2, 1).reshape(a["cout"], a["cin"], a["kh"], a["kw"]) for k, v in r.items()}
    d = T["dy_val"].double()
    return {"K": case.B * case.H * case.W,
            "dw": {"ref": r["acc"], "A": r["abs"], "R": r["sq"].sqrt(), "U": U_SMALL if small else U_MFMA},
            "db": {"ref": d.sum(0), "A": d.abs().sum(0), "R": (d * d).sum(0).sqrt(), "U": U_SUM}}


# ---------------------------------------------------------------------------------------------------------------------
# checks
# ---------------------------------------------------------------------------------------------------------------------
def compare(got, r, K, what, fails, mult=1.0):
    """got against mult * r["ref"] under mult x both bounds; appends messages to `fails`.  Returns the worst
    (|err| / per-element bound, |err| / aggregate bound): both <= 1 when the checks pass."""
    g = got.double()
    err = (g - mult * r["ref"]).abs()
    err = torch.where(torch.isfinite(g), err, torch.full_like(err, float("inf")))
    te = mult * C_ELEM * u_elem(r["U"], K) * r["A"]
    ta = mult * K_AGG * u_agg(r["U"], K) * r["R"]
    ratios = []
    for kind, tol in (("per-element", te), ("aggregate", ta)):
        ratio = float(torch.where(err > 0, err / tol.clamp_min(1e-300), torch.zeros_like(err)).max()) if err.numel() else 0.0
        ratios.append(ratio)
        bad = err > tol
        if bool(bad.any()):
            i = tuple(int(v) for v in torch.nonzero(bad)[0])
            fails.append(f"{what}: {int(bad.sum())} of {bad.numel()} elements beyond the {kind} bound (worst err/bound {ratio:.3g}), first at "
                         f"{i}: got {float(g[i]):.7g} want {float(mult * r['ref'][i]):.7g} bound {float(tol[i]):.3g}")
    return ratios[0], ratios[1]


def check_case(case: Case, ref: dict, mult: float = 1.0, db_mult=None):
    """All checks of one case after `mult` launches (db_mult launches with db; default mult): returns (failures,
    {"dw": (elem, agg), "db": (elem, agg)})."""
    a, T, K = case.launch.args, case.T, ref["K"]
    fails, worst = [], {"dw": (0.0, 0.0), "db": (0.0, 0.0)}
    cout = a["cout"]
    dw = T["dw"]
    if case.launch.kind == "mfma":
        cin = a["c0"] + a["c1"]
        worst["dw"] = compare(dw[:cout, :, :cin], ref["dw"], K, "dw", fails, mult)
        live = torch.zeros(dw.shape, dtype=torch.bool, device=dw.device)
        live[:cout, :, :cin] = True
        if not torch.equal(dw[~live], T["dw_init"][~live]):
            n = int((dw[~live] != T["dw_init"][~live]).sum())
            fails.append(f"dw: {n} padding elements (rows >= {cout} or columns >= {cin}) were written")
    else:
        worst["dw"] = compare(dw, ref["dw"], K, "dw", fails, mult)
    if "db" in T:
        worst["db"] = compare(T["db"][:cout], ref["db"], K, "db", fails, mult if db_mult is None else db_mult)
        if not torch.equal(T["db"][cout:], T["db_init"][cout:]):
            fails.append(f"db: elements past cout = {cout} were written")
    for name, off, c in (("x0", a.get("off0"), a.get("c0")), ("x1", a.get("off1"), a.get("c1")), ("dy", a["off_dy"], cout),
                         ("x", a.get("off_in"), a.get("cin"))):
        buf = T.get(name)
        if buf is None or buf.dim() != 2:
            continue
        keep = torch.ones(buf.shape[1], dtype=torch.bool, device=buf.device)
        keep[off:off + c] = False
        vals = T["dy_val"] if name == "dy" else None
        if not bool((buf[:, keep] == SENT_IN).all()) or (vals is not None and not torch.equal(buf[:, off:off + c], vals)):
            fails.append(f"{name}: an input buffer was written")
    return fails, worst
