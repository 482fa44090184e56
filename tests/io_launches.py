"""Launch-level checks of the kernels before the encoders and after the last iteration -- the sample grid and the input stage,
the evaluation metrics and their region sums, the weight traffic of a training step (pack, batched pack, unpack) and the layout
plumbing -- against float64 (not a conftest, nothing here is collected).  The same cases run on the CPU against the host emulation
of csrc/pf_elem.h (tests/test_io_launch_reference.py) and on the GPU against the HIP library (tests/test_hip_io_launches.py), built
like tests/elem_launches.py, whose table, checker and bilinear bound are reused unchanged: every launch is compared element by
element with a float64 statement of the same formula on the SAME fp32 inputs upcast, under a bound counted per output element in
fp32 roundings, U = 2^-24 each (one rounding of v costs at most U |v|; a division or a square root is taken as 2 U, as there).
No element is excluded from any comparison; a non-finite output for finite input fails (`ratio` returns inf).

Device libm.  sinf / cosf / asinf / acosf / atan2f / tanhf get a named allowance in ulp, ULP_* below, from the table "Relative
error as ULPs" of the OpenCL C specification (section 7.4, full profile), which OCML -- the device library hipcc links these
calls to -- is specified to; the ROCm installation carries no accuracy table of its own.  n ulp of a result v are at most
2 n U |v|.  None of them is fitted to an output: a ratio above 1 that only such a constant explains is reported in DESIGN.md with
the measured ulp, not widened here.

Through an inverse function the error d of the argument is carried as an interval, max |f(a +- d) - f(a)| with f the float64
function on the clamped argument: honest at asin(1), acos(+-1), where a derivative would blow up.

pf_sample_grid     (ref_sample_grid: the roundings of every line are counted next to it)
pf_img_rotate      zero-padded bilinear bound of elem_launches: pf_pymod (U W for -W < x < 0), pf_roundtrip (rt_err), M_BILIN;
                   the grid is an INPUT, so the wrapped coordinate never crosses the seam by rounding (W - tiny rounds to W, where
                   the zero-padded sample is continuous: 0 either way); a NaN coordinate gives exactly 0
pf_flow_metrics    (ref_metrics)
pf_region_sums     float64 sums per chunk; n U64 sum |term| for n terms in any order, U64 |s w| per product
pack / unpack      bit for bit against numpy (pack), U |scale dw| + U |result| (unpack: one product, one sum, fused or not)
layout             exact, except tanh: 2 ULP_TANH U |tanh|
"""
import math
from collections import OrderedDict

import numpy as np
import torch

import golden_cases as gc
from elem_launches import (K_MAX_BLOCKS, M_BILIN, SENT_F32, U, U64, Run, Table, bilin0, ratio, rt_err,  # noqa: F401  (re-exported)
                           taps0)

# OpenCL C specification, section 7.4 "Relative error as ULPs", full profile (what OCML's f32 functions are specified to)
ULP_SIN, ULP_COS, ULP_ASIN, ULP_ACOS, ULP_ATAN2, ULP_TANH = 4, 4, 4, 4, 6, 5
E_SIN, E_COS, E_ASIN, E_ACOS, E_ATAN2, E_TANH = (2.0 * n * U for n in (ULP_SIN, ULP_COS, ULP_ASIN, ULP_ACOS, ULP_ATAN2, ULP_TANH))

PI32 = float(np.float32(np.pi))            # 3.14159274101257324: the kernels' fp32 PI (both spellings in pf_elem.h round to it)
TWO_PI32 = float(np.float32(2 * np.pi))    # 6.28318548202514648 = 2 PI32 exactly
EPS_NUDGE = float(np.float32(1e-6))

LOOP = 256 * K_MAX_BLOCKS                  # a launch of one element per thread starts its second grid-stride trip here
SHAPES = OrderedDict(even=(2, 16, 32), ragged=(3, 17, 27), w4=(1, 12, 28), eval=(1, 64, 128))
H8W28 = (1, 8, 28)                         # H % 8 == 0, W % 8 != 0: still the raster order of pf_prepare_images
ROWS_PIX = (1, 2049, 2048)                 # B * H * W = LOOP + 2048: one element per pixel
ROWS_IMG = (1, 1024, 1368)                 # B * 3 * H * W = LOOP + 8192: one element per (plane, pixel); (H | W) & 7 == 0
ROWS_CL = (1, 1024, 820)                   # B * N * 5 = LOOP + 4096: pf_to_channel_last / pf_to_nchw with c = 5
assert ROWS_PIX[1] * ROWS_PIX[2] > LOOP and 3 * ROWS_IMG[1] * ROWS_IMG[2] > LOOP and 5 * ROWS_CL[1] * ROWS_CL[2] > LOOP


def dims(shape, rows=ROWS_PIX):
    return rows if shape == "rows" else (H8W28 if shape == "h8w28" else SHAPES[shape])


def same_bits(run, kernel, what, got, ref):
    """Bit identity of two tensors of one dtype (NaN payloads and the sign of zero included)."""
    it = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[got.element_size()]
    ok = got.dtype == ref.dtype and got.shape == ref.shape and torch.equal(got.contiguous().view(it), ref.contiguous().view(it))
    run.table.add(kernel, run.shape, 0.0 if ok else float("inf"))
    if not ok:
        run.fails.append(f"{kernel} [{run.shape}] {what}: not bit-identical")
    return ok


def guarded(shape, dev, fill=SENT_F32, guard=1):
    """A tensor of `shape` between `guard` sentinel slices along dim 0: (whole, view)."""
    whole = torch.full((shape[0] + 2 * guard,) + tuple(shape[1:]), fill, device=dev)
    return whole, whole[guard:-guard]


def guards_of(whole, guard=1):
    return torch.cat([whole[:guard].reshape(-1), whole[-guard:].reshape(-1)])


# ------------------------------------------------------------------------------------------------------------------------
# family: grid  (pf_sample_grid)
# ------------------------------------------------------------------------------------------------------------------------
def rot_xyz(ax, ay, az):
    cx, sx, cy, sy, cz, sz = math.cos(ax), math.sin(ax), math.cos(ay), math.sin(ay), math.cos(az), math.sin(az)
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return torch.from_numpy((rz @ ry @ rx).astype(np.float32))


def rotations():
    """Rx(+-pi/2) (the model's two views), the identity, one general rotation: fp32 matrices, as the entry point takes them."""
    return OrderedDict(a2b=rot_xyz(-math.pi / 2, 0, 0), b2a=rot_xyz(math.pi / 2, 0, 0), identity=torch.eye(3), general=rot_xyz(1.1, -0.7, 0.3))


def _nudge64(t):
    return torch.where(t.abs() < EPS_NUDGE, t + torch.sign(t) * EPS_NUDGE, t)


def _asin_iv(z, d):
    """asin of z known to +-d: value, max |asin(clamp(z +- d)) - asin(z)|."""
    f = lambda t: torch.asin(t.clamp(-1.0, 1.0))      # noqa: E731
    v = f(z)
    return v, torch.maximum((f(z + d) - v).abs(), (f(z - d) - v).abs())


def ref_sample_grid(H, W, R, dev, mut=None):
    """float64 restatement of pf_sample_grid_elem on the fp32 matrix R: (grid [2,H,W], bound [2,H,W], cut [H,W]).  `cut` marks
    the pixels on the +-pi cut of atan2 (yr within its error of 0, xr < 0), where m2 is compared modulo W."""
    Rd = R.double().reshape(9).tolist()
    m = torch.arange(W, dtype=torch.float64, device=dev).view(1, W).expand(H, W)
    n = torch.arange(H, dtype=torch.float64, device=dev).view(H, 1).expand(H, W)
    u = (m + 0.5) / W                                   # m + 0.5 exact; the division 2 U u
    theta = ((u - 0.5) * 2.0) * PI32                    # u - 0.5: U |u - 0.5|; * 2 exact; * PI: U |theta|
    e_th = 2.0 * PI32 * (2 * U * u + U * (u - 0.5).abs()) + U * theta.abs()
    v = (n + 0.5) / H
    phi = (0.5 - v) * PI32
    e_ph = PI32 * (2 * U * v + U * (0.5 - v).abs()) + U * phi.abs()
    cp, ct, st, z = torch.cos(phi), torch.cos(theta), torch.sin(theta), torch.sin(phi)
    e_cp, e_ct, e_st, e_z = e_ph + E_COS * cp.abs(), e_th + E_COS * ct.abs(), e_th + E_SIN * st.abs(), e_ph + E_SIN * z.abs()
    x, y = cp * ct, cp * st                             # a product: both factors' errors and one rounding
    e_x = e_cp * ct.abs() + cp.abs() * e_ct + e_cp * e_ct + U * x.abs()
    e_y = e_cp * st.abs() + cp.abs() * e_st + e_cp * e_st + U * y.abs()

    def row(i):                                         # (R0 x + R1 y) + R2 z: three products, two sums
        a, b, c = Rd[3 * i] * x, Rd[3 * i + 1] * y, Rd[3 * i + 2] * z
        val = (a + b) + c
        err = abs(Rd[3 * i]) * e_x + abs(Rd[3 * i + 1]) * e_y + abs(Rd[3 * i + 2]) * e_z + U * (a.abs() + b.abs() + c.abs()) + \
            U * (a + b).abs() + U * val.abs()
        return val, err

    (xr, e_xr), (yr, e_yr), (zr, e_zr) = row(0), row(1), row(2)
    phi2, e_p2 = _asin_iv(zr, e_zr)
    e_p2 = e_p2 + E_ASIN * (phi2.abs() + e_p2)
    # pf_nudge jumps by eps where |t| crosses eps and by 2 eps where t changes sign: the whole jump where float64 |t| is within
    # its error of either; the addition t + sgn eps is one more rounding (of at most 2 eps)
    jump = lambda t, e: ((t.abs() - EPS_NUDGE).abs() <= e) | (t.abs() <= e)          # noqa: E731
    e_xn = e_xr + 2 * EPS_NUDGE * jump(xr, e_xr) + 2 * U * EPS_NUDGE
    e_yn = e_yr + 2 * EPS_NUDGE * jump(yr, e_yr) + 2 * U * EPS_NUDGE
    xn, yn = _nudge64(xr), _nudge64(yr)
    theta2 = torch.atan2(yn, xn)
    hyp = (torch.hypot(xn, yn) - (e_xn + e_yn)).clamp_min(1e-300)                    # |d atan2| <= |d| / hypot
    e_t2 = (e_xn + e_yn) / hyp
    e_t2 = e_t2 + E_ATAN2 * (theta2.abs() + e_t2)
    cut = (yr.abs() <= e_yr + 2 * EPS_NUDGE) & (xr - e_xr < 0)
    if mut == "sign":                                   # the deliberate mistake: both angles with the other sign
        theta2, phi2 = -theta2, -phi2
    q = theta2 / TWO_PI32                               # 2 U |q|
    s = q + 0.5                                         # U |s|
    p = s * W                                           # U |p|
    m2 = p - 0.5                                        # U |m2|
    e_m2 = W * (e_t2 / TWO_PI32 + 2 * U * q.abs() + U * s.abs()) + U * p.abs() + U * m2.abs()
    q = phi2 / PI32
    s = 0.5 - q
    p = s * H
    n2 = p - 0.5
    e_n2 = H * (e_p2 / PI32 + 2 * U * q.abs() + U * s.abs()) + U * p.abs() + U * n2.abs()
    return torch.stack([m2, n2]), torch.stack([e_m2, e_n2]), cut


def cmp_grid(run, what, got, ref, bnd, cut, W):
    """m2 modulo W on the cut and nowhere else; n2 as it is."""
    g = got.double()
    d = g[0] - ref[0]
    alt = torch.where((d - W).abs() < (d + W).abs(), d - W, d + W)
    g0 = torch.where(cut & (alt.abs() < d.abs()), ref[0] + alt, g[0])
    return run.cmp("sample_grid", what, torch.stack([g0, g[1]]), ref, bnd)


def run_grid(lib, shape, dev, run):
    _, H, W = dims(shape)
    for name, R in rotations().items():
        if shape == "rows" and name != "general":
            continue
        whole, out = guarded((2, H, W), dev)
        lib.sample_grid(out, R)
        ref, bnd, cut = ref_sample_grid(H, W, R, dev)
        cmp_grid(run, name, out, ref, bnd, cut, W)
        run.sentinel("sample_grid", "planes around the grid", guards_of(whole))
        if name == "identity":                          # the identity rotation is coords_grid, within the very same bound
            ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64, device=dev), torch.arange(W, dtype=torch.float64, device=dev),
                                    indexing="ij")
            cg = torch.stack([xs, ys])
            cmp_grid(run, "identity is coords_grid", out, cg, bnd + (ref - cg).abs(), cut, W)


# ------------------------------------------------------------------------------------------------------------------------
# family: rotate  (pf_img_rotate)
# ------------------------------------------------------------------------------------------------------------------------
def nasty_grid(tag, H, W, dev):
    """gc.nasty_coords as a sampling grid: seam crossers, rows outside the map, negatives, multi-wrap x -- and one NaN."""
    g = gc.nasty_coords(tag, 1, H, W)[0].clone()
    g[0, H // 2, W // 3] = float("nan")
    g[1, H // 2 + 1, W // 2] = float("nan")
    return g.contiguous().to(dev)


def ref_img_rotate(img, grid, mut=None):
    """img [B,C,H,W] fp32, grid [2,H,W] fp32 -> float64 (out, bound)."""
    B, Cc, H, W = img.shape
    N = H * W
    gx, gy = grid[0].double().reshape(1, N), grid[1].double().reshape(1, N)
    bad = torch.isnan(gx) | torch.isnan(gy)
    gx, gy = torch.where(bad, torch.full_like(gx, -3.0 * W), gx), torch.where(bad, torch.full_like(gy, -3.0 * H), gy)
    x = torch.remainder(gx, W)
    dx = U * W * ((gx < 0) & (gx > -W)) + rt_err(x, W)
    dy = rt_err(gy, H)
    if mut == "clamp":                                  # the deliberate mistake: border clamp instead of zero padding
        x, gy = x.clamp(0, W - 1), gy.clamp(0, H - 1)
    maps = img.double().reshape(B * Cc, N)
    e = lambda t: t.expand(B * Cc, N)                   # noqa: E731
    v, b, _ = bilin0(maps, H, W, e(x), e(gy), e(dx), e(dy))
    keep = ~e(bad)
    return (v * keep).view(B, Cc, H, W), (b * keep).view(B, Cc, H, W)


def real_grid(lib, H, W, dev, name="a2b"):
    """The A->B grid of the shape, made by pf_sample_grid and read back (the fp32 values the model samples at)."""
    return lib.sample_grid(torch.empty(2, H, W, device=dev), rotations()[name])


def run_rotate(lib, shape, dev, run):
    B, H, W = dims(shape, ROWS_IMG)
    gen = torch.Generator().manual_seed(21)
    grids = OrderedDict(real=real_grid(lib, H, W, dev))
    if shape != "rows":
        grids["nasty"] = nasty_grid(f"io/rot/{shape}", H, W, dev)
    for Cc in ((1, 3, 6) if shape != "rows" else (3,)):
        img = (torch.rand(B, Cc, H, W, generator=gen) * 4 - 2).to(dev)
        for kind, grid in grids.items():
            whole, out = guarded((B, Cc, H, W), dev)
            lib.img_rotate(img, grid, out)
            run.cmp("img_rotate", f"C={Cc}, {kind} grid", out, *ref_img_rotate(img, grid))
            run.sentinel("img_rotate", "images around the output", guards_of(whole))


# ------------------------------------------------------------------------------------------------------------------------
# family: prepare  (pf_normalise_images, pf_prepare_images, pf_prepare_frame)
# ------------------------------------------------------------------------------------------------------------------------
def norm255_np(t):
    """numpy's fp32 2 * (image / 255.0) - 1.0 (IEEE division): the reference's CPU arithmetic (core/prior_raft.py:121-122)."""
    r = (np.float32(2) * (t.cpu().numpy() / np.float32(255)) - np.float32(1)).astype(np.float32)
    return torch.from_numpy(r).to(t.device)


def tile_order(H, W, dev):
    """pixel visited by index i of pf_prepare_images when (H | W) & 7 == 0: 64 consecutive indices = one 8 x 8 tile."""
    i = torch.arange(H * W, device=dev)
    tile, inn, tpr = i >> 6, i & 63, W >> 3
    return ((tile // tpr) * 8 + (inn >> 3)) * W + (tile % tpr) * 8 + (inn & 7)


def run_prepare(lib, shape, dev, run, mut=None):
    B, H, W = dims(shape, ROWS_IMG)
    gen = torch.Generator().manual_seed(31)
    i1 = (torch.rand(B, 3, H, W, generator=gen) * 255).round().to(dev)
    i2 = (torch.rand(B, 3, H, W, generator=gen) * 300 - 20).to(dev)
    i1.view(-1)[:256] = torch.arange(256.0, device=dev)[:min(256, i1.numel())]      # every integer pixel value
    n1, n2 = norm255_np(i1), norm255_np(i2)
    # pf_normalise_images: bit for bit, a count that is no multiple of 4, sentinel batches on both sides of each destination
    cnt = i1.numel() - (1 if i1.numel() % 4 != 1 else 2)
    assert cnt % 4 != 0
    (wf1, f1), (wf2, f2), (wc1, c1) = (guarded((B, 3, H, W), dev) for _ in range(3))
    for with_c in (True, False):
        for t in (wf1, wf2, wc1):
            t.fill_(SENT_F32)
        lib._rc(lib._dll.pf_normalise_images(i1.data_ptr(), i2.data_ptr(), f1.data_ptr(), f2.data_ptr(), c1.data_ptr() if with_c else None,
                                             cnt, lib._stream(i1)), "pf_normalise_images")
        flat = lambda t: t.reshape(-1)                  # noqa: E731
        same_bits(run, "normalise_images", "image1", flat(f1)[:cnt], flat(n1)[:cnt])
        same_bits(run, "normalise_images", "image2", flat(f2)[:cnt], flat(n2)[:cnt])
        if with_c:
            same_bits(run, "normalise_images", "context copy", flat(c1)[:cnt], flat(n1)[:cnt])
        rest = [flat(f1)[cnt:], flat(f2)[cnt:], guards_of(wf1), guards_of(wf2), guards_of(wc1), flat(c1)[cnt:] if with_c else flat(c1)]
        run.sentinel("normalise_images", "past count and around the destinations", torch.cat(rest))
    grids = OrderedDict(real=real_grid(lib, H, W, dev))
    if shape != "rows":
        grids["nasty"] = nasty_grid(f"io/prep/{shape}", H, W, dev)
    for kind, grid in grids.items():
        # the two-launch statement: normalise, rotate the normalised pair, copy im1_B
        f_ref = torch.full((4 * B, 3, H, W), SENT_F32, device=dev)
        lib.normalise_images(i1, i2, f_ref[:B], f_ref[B:2 * B], None)
        lib.img_rotate(f_ref[:2 * B], grid, f_ref[2 * B:])
        c_ref = torch.cat([f_ref[:B], f_ref[2 * B:3 * B]])
        if mut == "raster":         # the deliberate mistake, in the REFERENCE: index i taken for pixel i where the kernel walks tiles
            assert not (H | W) & 7
            f_ref = f_ref.view(4 * B, 3, H * W)[:, :, tile_order(H, W, dev)].view(4 * B, 3, H, W).contiguous()
        # the float64 bound on the rotated halves, so that the bit identity is not two copies of one mistake
        r64 = [ref_img_rotate(n, grid) for n in (n1, n2)]
        for with_c in (True, False):
            wf, f = guarded((4 * B, 3, H, W), dev)
            wc, c = guarded((2 * B, 3, H, W), dev)
            lib.prepare_images(i1, i2, grid, f, c if with_c else None)
            same_bits(run, "prepare_images", f"img_f, {kind} grid", f, f_ref)
            run.cmp("prepare_images", f"im1_B against float64, {kind} grid", f[2 * B:3 * B], *r64[0])
            run.cmp("prepare_images", f"im2_B against float64, {kind} grid", f[3 * B:], *r64[1])
            if with_c:
                same_bits(run, "prepare_images", f"img_c, {kind} grid", c, c_ref)
            run.sentinel("prepare_images", "around the batches", torch.cat([guards_of(wf), guards_of(wc), c.reshape(-1)[:0 if with_c else None]]))
        wo, o = guarded((2 * B, 3, H, W), dev)
        lib.prepare_frame(i1, grid, o)
        same_bits(run, "prepare_frame", f"img_c of prepare_images, {kind} grid", o, c_ref)
        run.cmp("prepare_frame", f"im_B against float64, {kind} grid", o[B:], *r64[0])
        run.sentinel("prepare_frame", "around the batch", guards_of(wo))


# ------------------------------------------------------------------------------------------------------------------------
# family: metrics  (pf_flow_metrics)
# ------------------------------------------------------------------------------------------------------------------------
ROW_KINDS = ("random", "seam+", "seam-", "top", "bottom", "large", "equal", "antipodal", "coincident", "close")


def metric_flows(tag, B, H, W, seed):
    """pred, gt [4 B, 2, H, W] (or [1, 2, H, W] for B == 0).  Image i % 4 == 0 holds the rows of ROW_KINDS in turn: random flows;
    end points across the x seam in both directions and by several W; rows clamped at the top and at the bottom; |u| up to 1000;
    pred == gt bitwise; antipodal pairs; coincident end points reached by different flows; pairs 1e-3 px apart.  Image 1 is antipodal
    pairs over the whole image (gt = 0, pred = (W/2, H - 1 - 2y)), image 2 coincident ones (pred = gt + (W, 0); its even rows with
    gt = 0), image 3 a perfect prediction (pred == gt bitwise, random)."""
    gen = torch.Generator().manual_seed(seed)
    nimg = 4 * B if B else 1
    xs = torch.arange(W, dtype=torch.float32).view(1, W).expand(H, W)
    ys = torch.arange(H, dtype=torch.float32).view(H, 1).expand(H, W)
    r = lambda s=12.0: (torch.rand(2, H, W, generator=gen) - 0.5) * s        # noqa: E731
    anti = torch.stack([torch.full((H, W), W / 2.0), H - 1 - 2 * ys])
    preds, gts = [], []
    for i in range(nimg):
        gt, pred = r(), r()
        kind = i % 4
        if kind == 0:
            K = len(ROW_KINDS)
            k = lambda name: slice(ROW_KINDS.index(name), None, K)            # noqa: E731
            pred[0, k("seam+")] = (W - xs[k("seam+")]) + torch.rand(xs[k("seam+")].shape, generator=gen) + W * 2.0      # ends right of the seam, 2 W on
            gt[0, k("seam+")] = (W - xs[k("seam+")]) - torch.rand(xs[k("seam+")].shape, generator=gen)                  # ends left of it
            pred[0, k("seam-")] = -xs[k("seam-")] - torch.rand(xs[k("seam-")].shape, generator=gen) - W * 3.0
            gt[0, k("seam-")] = -xs[k("seam-")] + torch.rand(xs[k("seam-")].shape, generator=gen)
            pred[0, k("seam-"), ::3] = -xs[k("seam-"), ::3] - 0.5             # x + u + 0.5 == 0 exactly, and a tiny negative beside it
            pred[0, k("seam-"), 1::3] = -xs[k("seam-"), 1::3] - 0.5 - 2.0 ** -20
            pred[1, k("top")] = -ys[k("top")] - 3.0 * torch.rand(ys[k("top")].shape, generator=gen)
            gt[1, k("top")] = -ys[k("top")] - 0.5                            # on the clamp value itself
            pred[1, k("bottom")] = (H - ys[k("bottom")]) + 5.0 * torch.rand(ys[k("bottom")].shape, generator=gen) - 0.5
            gt[1, k("bottom")] = 2.0 * H
            pred[:, k("large")] = (torch.rand(pred[:, k("large")].shape, generator=gen) - 0.5) * 2000.0
            gt[:, k("large")] = (torch.rand(gt[:, k("large")].shape, generator=gen) - 0.5) * 2000.0
            pred[:, k("equal")] = gt[:, k("equal")]
            gt[:, k("antipodal")] = 0.0
            pred[:, k("antipodal")] = anti[:, k("antipodal")]
            pred[:, k("coincident")] = gt[:, k("coincident")]
            pred[0, k("coincident")] += W
            pred[:, k("close")] = gt[:, k("close")] + 1e-3 * (torch.rand(gt[:, k("close")].shape, generator=gen) - 0.5)
        elif kind == 1:
            gt, pred = torch.zeros(2, H, W), anti.clone()
        elif kind == 2:
            gt[:, ::2] = 0.0
            pred = gt.clone()
            pred[0] += W
        else:
            pred = gt.clone()
        preds.append(pred)
        gts.append(gt)
    return torch.stack(preds).contiguous(), torch.stack(gts).contiguous()


def _endpoint64(x, y, u, v, H, W, mut=None):
    """float64 pf_endpoint_sph: theta, phi, their error bounds, and whether fp32 may wrap x on the other side of a multiple of W."""
    s = x + u                                           # U |s|
    a = s + 0.5                                         # U |a|
    e_a = U * (s.abs() + a.abs())
    wraps = (a - W * torch.round(a / W)).abs() <= e_a
    neg = (a < 0) & (a > -W)                            # pf_pymod: one rounding of magnitude <= W there, exact elsewhere
    mm = a if mut == "x_not_wrapped" else torch.remainder(a, W)
    e0 = mm - 0.5                                       # U |e0|
    t1 = e0 + 0.5                                       # U |t1|
    q = t1 / W                                          # 2 U |q|: 2 U |t1| in pixels
    t3 = q - 0.5                                        # U |t3|, U |theta| after the factor 2 pi
    th = (t3 * 2.0) * PI32                              # U |theta|
    e_th = (2.0 * PI32 / W) * (e_a + U * W * neg + U * e0.abs() + 3 * U * t1.abs()) + 2 * U * th.abs()
    e1 = y + v                                          # U |e1|, which the clamp removes where e1 is beyond it by more than that
    lo, hi = -0.5, H - 0.5
    e_e1 = U * e1.abs() * ((e1 > lo - U * e1.abs()) & (e1 < hi + U * e1.abs()))
    e1c = e1 if mut == "y_not_clamped" else e1.clamp(lo, hi)
    t = e1c + 0.5                                       # U |t|
    q = t / H                                           # 2 U |t| in pixels
    r = 0.5 - q                                         # U |r|, U |phi| after the factor pi
    ph = r * PI32                                       # U |phi|
    e_ph = (PI32 / H) * (e_e1 + 3 * U * t.abs()) + 2 * U * ph.abs()
    return th, ph, e_th, e_ph, wraps


def ref_metrics(pred, gt, mut=None):
    """float64 pf_flow_metrics_elem: dict of (value, bound) [B,H,W] for epe, hav (Haversine form) and cos (Cosine form)."""
    B, _, H, W = pred.shape
    dev = pred.device
    p, g = pred.double(), gt.double()
    x = torch.arange(W, dtype=torch.float64, device=dev).view(1, 1, W)
    y = torch.arange(H, dtype=torch.float64, device=dev).view(1, H, 1)
    # EPE: du, dv one rounding each and twice in their squares (2), the squares (1), the sum (1): 4 U of the radicand, 2 U of the
    # root, and sqrtf's own 2 U
    du, dv = p[:, 0] - g[:, 0], p[:, 1] - g[:, 1]
    epe = torch.sqrt(du * du + dv * dv)
    out = dict(epe=(epe, 4 * U * epe))
    tp, pp, e_tp, e_pp, wp = _endpoint64(x, y, p[:, 0], p[:, 1], H, W, mut)
    tg, pg, e_tg, e_pg, wg = _endpoint64(x, y, g[:, 0], g[:, 1], H, W, mut)
    # tg - tp: fp32 may have wrapped one end point to the other side of the seam, which moves the difference by 2 PI32: the
    # rounding is charged at |tp| + |tg| (either branch), and 2 PI32 is 2 (PI32 - pi) off a period of sin^2(./2) and cos
    dth = (tp + tg) if mut == "theta_sum" else (tg - tp)
    e_dth = e_tp + e_tg + U * (tp.abs() + tg.abs()) + 2 * abs(PI32 - math.pi) * (wp | wg)
    cp, cg = torch.cos(pp), torch.cos(pg)
    e_cp, e_cg = e_pp + E_COS * cp.abs(), e_pg + E_COS * cg.abs()
    cc = cp * cg
    e_cc = e_cp * cg.abs() + cp.abs() * e_cg + e_cp * e_cg + U * cc.abs()
    same = (pred[:, 0] == gt[:, 0]) & (pred[:, 1] == gt[:, 1])
    # Haversine form
    dph = pg - pp
    e_dph = e_pp + e_pg + U * dph.abs()
    s1, s2 = torch.sin(dph / 2), torch.sin(dth / 2)                  # x / 2 is exact
    e_s1, e_s2 = e_dph / 2 + E_SIN * s1.abs(), e_dth / 2 + E_SIN * s2.abs()
    h1, h2 = s1 * s1, s2 * s2
    e_h1, e_h2 = 2 * s1.abs() * e_s1 + e_s1 ** 2 + U * h1, 2 * s2.abs() * e_s2 + e_s2 ** 2 + U * h2
    prod = cc * h2
    hv = h1 + prod
    d = e_h1 + e_cc * h2 + cc.abs() * e_h2 + e_cc * e_h2 + U * prod.abs() + U * hv.abs()
    d = d + 4 * U * hv.abs()                            # sqrtf: 2 U of the root is 4 U of its argument
    f = lambda t: 2.0 * torch.asin(torch.sqrt(t.clamp(0.0, 1.0)))    # noqa: E731
    sd = f(hv)
    up = f(hv + d)
    bnd = torch.maximum(up - sd, sd - f(hv - d)) + E_ASIN * up
    out["hav"] = (sd, torch.where(same, torch.zeros_like(bnd), bnd))  # pred == gt bitwise: every difference is exactly 0
    # Cosine form
    sp, sg = torch.sin(pp), torch.sin(pg)
    e_sp, e_sg = e_pp + E_SIN * sp.abs(), e_pg + E_SIN * sg.abs()
    ss = sp * sg
    e_ss = e_sp * sg.abs() + sp.abs() * e_sg + e_sp * e_sg + U * ss.abs()
    cd = torch.cos(dth)
    e_cd = e_dth + E_COS * cd.abs()
    prod = cc * cd
    ca = ss + prod
    d = e_ss + e_cc * cd.abs() + cc.abs() * e_cd + e_cc * e_cd + U * prod.abs() + U * ca.abs()
    f = lambda t: torch.acos(t.clamp(-1.0, 1.0))        # noqa: E731
    sd = f(ca)
    lo_v, hi_v = f(ca + d), f(ca - d)                   # acos decreases
    out["cos"] = (sd, torch.maximum(sd - lo_v, hi_v - sd) + E_ACOS * hi_v)
    return out


def run_metrics(lib, shape, dev, run):
    B, H, W = dims(shape)
    pred, gt = metric_flows(f"io/met/{shape}", 0 if shape == "rows" else B, H, W, seed=41)
    pred, gt = pred.to(dev), gt.to(dev)
    ref = ref_metrics(pred, gt)
    nb = pred.shape[0]
    for cosine, key in ((False, "hav"), (True, "cos")):
        kernel = "flow_metrics_" + key
        for want_epe, want_sd in ((True, True), (True, False), (False, True)):
            we, epe = guarded((nb, H, W), dev)
            ws, sd = guarded((nb, H, W), dev)
            lib.flow_metrics(pred, gt, epe if want_epe else None, sd if want_sd else None, cosine)
            tag = "both" if want_epe and want_sd else "alone"
            if want_epe:
                run.cmp("flow_metrics_epe", f"epe, {tag}", epe, *ref["epe"])
            if want_sd:
                run.cmp(kernel, f"sd, {tag}", sd, *ref[key])
            run.sentinel(kernel, "images around the outputs and an output not asked for",
                         torch.cat([guards_of(we), guards_of(ws), epe.reshape(-1)[:0 if want_epe else None], sd.reshape(-1)[:0 if want_sd else None]]))


# ------------------------------------------------------------------------------------------------------------------------
# family: region  (pf_region_sums)
# ------------------------------------------------------------------------------------------------------------------------
SENT_F64 = -4321.25


def region_case(N, dev, B=3, seed=51):
    gen = torch.Generator().manual_seed(seed)
    c = dict(N=N, B=B)
    c["epe"] = (torch.rand(B, N, generator=gen) * 30).to(dev)
    c["sd"] = (torch.rand(B, N, generator=gen) * 3.2).to(dev)
    c["weight"] = (torch.rand(N, generator=gen) / N).to(dev)
    bits = torch.randint(0, 256, (N,), generator=gen, dtype=torch.int32)
    bits[::5] = 0                                       # pixels in no region
    bits[1::7] = 0x80 | 0x10                            # only bits at or above nregions = 1 / 3 set
    c["bits"] = bits.to(torch.uint8).to(dev)
    return c


def ref_region(c, nblk, R, with_w, mut=None):
    B, N = c["B"], c["N"]
    dev = c["epe"].device
    chunk = -(-N // nblk)
    blk = torch.arange(N, device=dev) // chunk
    e, s = c["epe"].double(), c["sd"].double()
    w = c["weight"].double() if with_w else (torch.ones(N, dtype=torch.float64, device=dev) if mut == "weight_one" else torch.zeros(N, dtype=torch.float64, device=dev))
    terms = torch.stack([e, s, s * w], 2)                                     # [B, N, 3]
    ref = torch.zeros(B, nblk, R, 3, dtype=torch.float64, device=dev)
    mag = torch.zeros_like(ref)
    cnt = torch.zeros(nblk, R, dtype=torch.float64, device=dev)
    for r in range(R):
        inr = ((c["bits"].to(torch.int32) >> r) & 1).double()
        if mut == "drop_last":
            inr = inr * (blk != (N - 1) // chunk)
        ref[:, :, r].index_add_(1, blk, terms * inr.view(1, N, 1))
        mag[:, :, r].index_add_(1, blk, terms.abs() * inr.view(1, N, 1))
        cnt[:, r].index_add_(0, blk, inr)
    bnd = cnt.view(1, nblk, R, 1) * U64 * mag
    bnd[..., 2] += U64 * mag[..., 2]                                          # the products s * w
    return ref, bnd


def run_region(lib, shape, dev, run):
    if shape == "rows":
        N, B, configs = LOOP + 1027, 1, [(4096, 3, True), (64, 1, False)]       # one image: the chunks are what grows
    else:
        _, H, W = dims(shape)
        N, B = H * W, 3
        configs = [(nblk, R, w) for nblk in (1, 5, 64, N, N + 3, 4096) if nblk <= 4096 for R in (1, 3, 8) for w in (True, False)]
    c = region_case(N, dev, B)
    for nblk, R, with_w in configs:
        n = B * nblk * R * 3
        bufs = []
        for _ in range(2):
            flat = torch.full((n + 64,), SENT_F64, dtype=torch.float64, device=dev)
            part = flat[32:32 + n].view(B, nblk, R, 3)
            lib.region_sums(c["epe"], c["sd"], c["weight"] if with_w else None, c["bits"], R, part)
            bufs.append((flat, part))
        (flat, part), (_, again) = bufs
        what = f"nblk={nblk} R={R} weight={'given' if with_w else 'NULL'}"
        run.cmp("region_sums", what, part, *ref_region(c, nblk, R, with_w))
        same_bits(run, "region_sums", what + ", launched twice", again, part)
        if not with_w and float(part[..., 2].abs().max()) != 0.0:
            run.fails.append(f"region_sums [{run.shape}] {what}: the weighted sum is not exactly 0")
        if not bool((torch.cat([flat[:32], flat[32 + n:]]) == SENT_F64).all()):
            run.fails.append(f"region_sums [{run.shape}] {what}: wrote outside [B][nblk][nregions][3]")


# ------------------------------------------------------------------------------------------------------------------------
# family: pack  (pf_pack_conv_weights, pf_pack_conv_weights_batch)
# ------------------------------------------------------------------------------------------------------------------------
PACK_SHAPES = ((124, 0, 272, 3, 3), (128, 128, 384, 1, 5), (2, 0, 256, 3, 3), (576, 0, 256, 1, 1), (32, 0, 8, 3, 3), (64, 0, 3, 7, 7),
               (5, 3, 33, 5, 1))
PACK_ROWS = (1024, 0, 480, 3, 3)            # 1024 * 9 * 480 = LOOP + 229 376 elements
BF16_DIRTY = 0x7FC0
assert PACK_ROWS[0] * 9 * PACK_ROWS[2] > LOOP


def bf16_rne_np(v):
    """pf_bf16_rne on a float32 array: round to nearest even on the bits -> uint16."""
    u = v.view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFFFFFF) >> 16).astype(np.uint16)


def split_np(v, mut=None):
    """hi = bf16_rne(v), lo = bf16_rne(v - hi): uint16 arrays."""
    hi = bf16_rne_np(v)
    hif = (hi.astype(np.uint32) << 16).view(np.float32)
    if mut == "lo_unrounded":               # the deliberate mistake: lo from the truncated, not the rounded hi
        hif = (v.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    with np.errstate(all="ignore"):
        lo = bf16_rne_np((v - hif).astype(np.float32))
    return hi, lo


def special_values():
    """+-0, denormals, +-inf, a NaN, and bf16 rounding ties with the even neighbour below and above (and their negatives)."""
    bits = [0x00000000, 0x80000000, 0x00000001, 0x807FFFFF, 0x00008000, 0x7F800000, 0xFF800000, 0x7FC00000,
            0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F80C000, 0x3F804000, 0x7F7FFFFF, 0x00800000]
    return np.array(bits, dtype=np.uint32).view(np.float32)


def pack_weights(shape, seed):
    cout0, cout1, cin, kh, kw = shape
    rng = np.random.RandomState(seed)
    mk = lambda *s: (rng.rand(*s) * 2 - 1).astype(np.float32)          # noqa: E731
    w0, w1 = mk(cout0, cin, kh, kw), (mk(cout1, cin, kh, kw) if cout1 else None)
    sp = special_values()
    for w in (w0, w1):
        if w is not None:
            pos = rng.choice(w.size, size=min(w.size, 4 * len(sp)), replace=False)
            w.reshape(-1)[pos] = np.resize(sp, pos.size)
    return w0, w1, mk(cout0), (mk(cout1) if cout1 else None)


def ref_pack(w0, w1, b0, b1, mode, cin_rot, cout_pad, cin_pad, with_bias, mut=None):
    """numpy restatement of pf_pack_conv_weights_elem: (uint16 [cout_pad, taps, cin_pad / 32, 2, 32], fp32 bias [cout_pad] | None).
    mode 0: dst[o][tap][c] = W[o][c][tap];  mode 1: dst[o][tap][c] = W[c][(o + cin_rot) % cin][taps - 1 - tap]."""
    w = w0 if w1 is None else np.concatenate([w0, w1], 0)
    cout, cin, kh, kw = w.shape
    taps = kh * kw
    w = w.reshape(cout, cin, taps)
    P = np.zeros((cout_pad, taps, cin_pad), dtype=np.float32)
    if mode == 0:
        P[:cout, :, :cin] = w.transpose(0, 2, 1)
    else:
        rolled = np.roll(w, cin_rot if mut == "rot_direction" else -cin_rot, axis=1)       # rolled[:, o] = w[:, (o + rot) % cin]
        P[:cin, :, :cout] = (rolled if mut == "taps_not_flipped" else rolled[:, :, ::-1]).transpose(1, 2, 0)
    hi, lo = split_np(P, mut)
    dst = np.stack([hi.reshape(cout_pad, taps, cin_pad // 32, 32), lo.reshape(cout_pad, taps, cin_pad // 32, 32)], 3)
    bias = None
    if with_bias:
        bias = np.zeros(cout_pad, dtype=np.float32)
        if mode == 0:
            if b0 is not None:
                bias[:w0.shape[0]] = b0
            if b1 is not None:
                bias[w0.shape[0]:cout] = b1
    return dst, bias


def r_up(v, m):
    return (v + m - 1) // m * m


def pack_configs(shape):
    """(mode, cin_rot, cout_pad, cin_pad, bias variant) of one weight shape; bias variants: both, b0, b1, none (dst_b NULL)."""
    cout0, cout1, cin, kh, kw = shape
    cout = cout0 + cout1
    out = [(0, 0, r_up(cout, 128), r_up(cin, 32), "both"), (0, 0, r_up(cout, 128) + 128, r_up(cin, 32), "b0"),
           (0, 0, r_up(cout, 128), r_up(cin, 32) + 32, "b1"), (0, cin - 1, r_up(cout, 128), r_up(cin, 32), "none")]
    rots = sorted({0, 1 % cin, cin - 1} | ({128} if cin > 128 else set()))
    for i, rot in enumerate(rots):
        out.append((1, rot, r_up(cin, 4) if i % 2 == 0 else r_up(cin, 128), r_up(cout, 32), ("both", "none", "b0", "b1")[i % 4]))
    return out


class PackCall:
    """One pack problem on the device: its operands, a dirty destination between guard bands, its reference."""

    def __init__(self, shape, cfg, dev, seed):
        self.shape, self.cfg = shape, cfg
        mode, rot, cout_pad, cin_pad, bias = cfg
        cout0, cout1, cin, kh, kw = shape
        w0, w1, b0, b1 = pack_weights(shape, seed)
        if bias in ("b1", "none"):
            b0 = None
        if bias in ("b0", "none") or not cout1:
            b1 = None
        self.np_ops = (w0, w1, b0, b1)
        t = lambda a: None if a is None else torch.from_numpy(a).to(dev)         # noqa: E731
        self.w0, self.w1, self.b0, self.b1 = t(w0), t(w1), t(b0), t(b1)
        self.n = 2 * cout_pad * kh * kw * cin_pad       # bf16 words: hi and lo of every element
        self.G = 96
        self.with_bias = bias != "none"
        self.dirty(dev)

    def dirty(self, dev):
        cout_pad = self.cfg[2]
        self.dst_all = torch.full((self.n + 2 * self.G,), BF16_DIRTY, dtype=torch.int16, device=dev)
        self.dst = self.dst_all[self.G:self.G + self.n]
        self.b_all = torch.full((cout_pad + 8,), SENT_F32, device=dev)
        self.b_all[4:-4] = float("nan")
        self.b = self.b_all[4:-4]

    def args(self):
        cout0, cout1, cin, kh, kw = self.shape
        mode, rot, cout_pad, cin_pad, _ = self.cfg
        p = lambda t: None if t is None else t.data_ptr()                        # noqa: E731
        return (p(self.w0), cout0, p(self.w1), cout1, p(self.b0), p(self.b1), cin, kh, kw, mode, rot, self.dst.data_ptr(),
                p(self.b) if self.with_bias else None, cout_pad, cin_pad)

    def check(self, run, kernel, what, mut=None):
        mode, rot, cout_pad, cin_pad, _ = self.cfg
        w0, w1, b0, b1 = self.np_ops
        ref_w, ref_b = ref_pack(w0, w1, b0, b1, mode, rot, cout_pad, cin_pad, self.with_bias, mut)
        got = self.dst.cpu().numpy().view(np.uint16).reshape(ref_w.shape)
        # v - hi is inf - inf for an infinite weight: the NaN an addition produces has the platform's sign; any NaN matches a NaN
        isnan = lambda a: ((a & 0x7F80) == 0x7F80) & ((a & 0x007F) != 0)        # noqa: E731
        ok = bool(np.all((got == ref_w) | (isnan(got) & isnan(ref_w))))
        gb = self.b_all.cpu().numpy()
        if self.with_bias:
            ok_b = np.array_equal(gb[4:-4].view(np.uint32), ref_b.view(np.uint32))
        else:
            ok_b = bool(np.isnan(gb[4:-4]).all())
        guards = bool((self.dst_all[:self.G] == BF16_DIRTY).all()) and bool((self.dst_all[self.G + self.n:] == BF16_DIRTY).all()) and \
            bool((gb[:4] == SENT_F32).all()) and bool((gb[-4:] == SENT_F32).all())
        run.table.add(kernel, run.shape, 0.0 if ok and ok_b and guards else float("inf"))
        for good, msg in ((ok, "operand not bit-identical (padding included)"), (ok_b, "bias"), (guards, "wrote outside its destination")):
            if not good:
                run.fails.append(f"{kernel} [{run.shape}] {what}: {msg}")
        return ok and ok_b and guards


def run_pack(lib, shape, dev, run):
    """pf_pack_conv_weights through the raw entry point into a dirty destination."""
    shapes = (PACK_ROWS,) if shape == "rows" else PACK_SHAPES
    for si, ws in enumerate(shapes):
        for ci, cfg in enumerate(pack_configs(ws)[:2 if shape == "rows" else None]):
            call = PackCall(ws, cfg, dev, seed=100 * si + ci)
            lib._rc(lib._dll.pf_pack_conv_weights(*call.args(), lib._stream(call.w0)), "pf_pack_conv_weights")
            call.check(run, "pack_conv_weights", f"{ws} mode={cfg[0]} rot={cfg[1]} pad={cfg[2]}x{cfg[3]} bias={cfg[4]}")


BATCH_JOBS = 35
TINY_PACK = ((1, 0, 7, 1, 1), (0, 0, 1, 32, "both"))        # cout_pad * taps * cin_pad = 1 x 32 elements


def batch_calls(dev):
    """35 jobs (three launches, the last of 3) cycling through the shapes and the configurations above, one of them 1 x 32."""
    from prior_flow_amd._lib import PackJob
    calls = []
    for j in range(BATCH_JOBS):
        ws = PACK_SHAPES[j % len(PACK_SHAPES)]
        cfgs = pack_configs(ws)
        ws, cfg = (ws, cfgs[(j // len(PACK_SHAPES) + j) % len(cfgs)]) if j != 20 else TINY_PACK
        calls.append(PackCall(ws, cfg, dev, seed=500 + j))
    arr = (PackJob * len(calls))()
    for q, call in zip(arr, calls):
        (q.w0, q.cout0, q.w1, q.cout1, q.b0, q.b1, q.cin, q.kh, q.kw, q.mode, q.cin_rot, q.dst_w, q.dst_b, q.cout_pad, q.cin_pad) = call.args()
    return calls, arr


def run_pack_batch(lib, shape, dev, run):
    calls, arr = batch_calls(dev)
    lib._rc(lib._dll.pf_pack_conv_weights_batch(arr, len(calls), lib._stream(calls[0].w0)), "pf_pack_conv_weights_batch")
    batched = []
    for j, call in enumerate(calls):
        call.check(run, "pack_conv_weights_batch", f"job {j} {call.shape} {call.cfg}")
        batched.append((call.dst_all.clone(), call.b_all.clone()))
        call.dirty(dev)                                 # an equally dirty destination for the single pack
        lib._rc(lib._dll.pf_pack_conv_weights(*call.args(), lib._stream(call.w0)), "pf_pack_conv_weights")
        same_bits(run, "pack_conv_weights_batch", f"job {j} against its single pack", batched[-1][0], call.dst_all)
        same_bits(run, "pack_conv_weights_batch", f"job {j} bias against its single pack", batched[-1][1], call.b_all)


# ------------------------------------------------------------------------------------------------------------------------
# family: unpack  (pf_unpack_wgrads)
# ------------------------------------------------------------------------------------------------------------------------
UNPACK_SHAPES = ((64, 3, 7, 7, 0), (128, 384, 1, 5, 128), (2, 256, 3, 3, 0), (576, 256, 1, 1, 0), (128, 272, 3, 3, 0), (5, 33, 5, 1, 4))
UNPACK_ROWS = ((1024, 480, 3, 3, 0),)       # cout * cin * taps = LOOP + 229 376
SCALES = (1.0, 0.25, float(np.float32(1.0 / 3.0)))


def unpack_case(shapes, njobs, dev, seed=61):
    """jobs over `shapes` in turn.  dw rows outside [o_off, o_off + cout) and columns at or past cin, and db outside its slice, are
    NaN; gw / gb are views into ONE flat buffer with sentinel floats between them (the optimiser's flat gradient buffer); job 3 has
    gb NULL and db given."""
    gen = torch.Generator().manual_seed(seed)
    specs, total = [], 7
    for j in range(njobs):
        cout, cin, kh, kw, o_off = shapes[j % len(shapes)]
        specs.append((cout, cin, kh, kw, o_off, total, total + cout * cin * kh * kw + 5))
        total += cout * cin * kh * kw + 5 + cout + 3
    flat = torch.full((total,), SENT_F32, device=dev)
    used = torch.zeros(total, dtype=torch.bool, device=dev)
    jobs, meta = [], []
    for j, (cout, cin, kh, kw, o_off, a, b) in enumerate(specs):
        taps, cin_pad = kh * kw, r_up(cin, 32)
        op = r_up(o_off + cout, 128)
        dw = torch.full((op, taps, cin_pad), float("nan"))
        dw[o_off:o_off + cout, :, :cin] = torch.randn(cout, taps, cin, generator=gen)
        db = torch.full((op,), float("nan"))
        db[o_off:o_off + cout] = torch.randn(cout, generator=gen)
        dw, db = dw.to(dev), db.to(dev)
        gw = flat[a:a + cout * cin * taps].view(cout, cin, kh, kw)
        gw.copy_(torch.randn(cout, cin, kh, kw, generator=gen))
        used[a:a + gw.numel()] = True
        gb = None
        if j != 3:
            gb = flat[b:b + cout]
            gb.copy_(torch.randn(cout, generator=gen))
            used[b:b + cout] = True
        scale = SCALES[j % 3]
        jobs.append((dw, db, gw, gb, cout, cin, taps, cin_pad, o_off, scale))
        meta.append((gw.clone(), None if gb is None else gb.clone()))
    return dict(jobs=jobs, before=meta, flat=flat, used=used)


def ref_unpack(job, before, mut=None):
    """float64 gw + scale * dw[o_off + o][tap][c] and gb + scale * db[o_off + o]; bound U |scale dw| + U |result| (the product and
    the sum: a fused multiply-add rounds once, inside the same bound)."""
    dw, db, gw, gb, cout, cin, taps, cin_pad, o_off, scale = job
    gw0, gb0 = before
    off = 0 if mut == "no_o_off" else o_off
    d = dw.double()
    if mut == "cin_stride":                 # the deliberate mistake: rows of cin, not cin_pad, floats
        d = d.reshape(-1)[:(d.numel() // cin) * cin].view(-1, cin)[off * taps:(off + cout) * taps].reshape(cout, taps, cin)
    else:
        d = d[off:off + cout, :, :cin]
    add = scale * d.permute(0, 2, 1).reshape(gw0.shape)
    rw = gw0.double() + add
    out = [(rw, U * add.abs() + U * rw.abs())]
    if gb0 is not None:
        addb = scale * db.double()[off:off + cout]
        rb = gb0.double() + addb
        out.append((rb, U * addb.abs() + U * rb.abs()))
    return out


def run_unpack(lib, shape, dev, run):
    c = unpack_case(UNPACK_ROWS, 1, dev) if shape == "rows" else unpack_case(UNPACK_SHAPES, BATCH_JOBS, dev)
    lib.unpack_wgrads(c["jobs"])
    for j, (job, before) in enumerate(zip(c["jobs"], c["before"])):
        refs = ref_unpack(job, before)
        run.cmp("unpack_wgrads", f"job {j} gw", job[2], *refs[0])
        if job[3] is not None:
            run.cmp("unpack_wgrads", f"job {j} gb", job[3], *refs[1])
    run.sentinel("unpack_wgrads", "the floats between the gradients", c["flat"][~c["used"]])


# ------------------------------------------------------------------------------------------------------------------------
# family: layout  (pf_to_channel_last, pf_to_nchw, pf_space_to_depth2, pf_flow_prep)
# ------------------------------------------------------------------------------------------------------------------------
def ref_to_channel_last(x, c_begin, c, act, mut=None):
    B, Ct, H, W = x.shape
    if mut == "no_c_begin":
        c_begin = 0
    v = x[:, c_begin:c_begin + c].double().permute(0, 2, 3, 1).reshape(B * H * W, c)
    if act == 1:
        return torch.where(v > 0, v, torch.zeros_like(v)), 0.0          # fmaxf(v, 0)
    if act == 2:
        t = torch.tanh(v)
        return t, E_TANH * t.abs()
    return v, 0.0


def ref_s2d(x, mut=None):
    """out[b][Y][X][(py * 2 + px) * C + c] = in[b][c][2 Y + py][2 X + px]"""
    B, Cc, H, W = x.shape
    v = x.double().view(B, Cc, H // 2, 2, W // 2, 2)                      # b c Y py X px
    order = (0, 2, 4, 5, 3, 1) if mut == "py_px" else (0, 2, 4, 3, 5, 1)
    return v.permute(*order).reshape(B * (H // 2) * (W // 2), 4 * Cc)


def run_layout(lib, shape, dev, run):
    gen = torch.Generator().manual_seed(71)
    B, H, W = dims(shape, ROWS_CL)
    N = H * W
    Ct, c_begin, c, ld, off = (12, 3, 5, 11, 2) if shape != "rows" else (6, 1, 5, 8, 2)
    x = (torch.randn(B, Ct, H, W, generator=gen) * 2).to(dev)
    for act in (0, 1, 2):
        out = torch.full((B * N, ld), SENT_F32, device=dev)
        lib.to_channel_last(x, c_begin, c, out, off, act)
        run.cmp("to_channel_last", f"act={act}", out[:, off:off + c], *ref_to_channel_last(x, c_begin, c, act))
        run.sentinel("to_channel_last", "columns on both sides", torch.cat([out[:, :off], out[:, off + c:]], 1))
        if act == 0:
            rows = out
    # pf_to_nchw of the rows just written: the slice comes back, and it is the input's
    whole, back = guarded((B, c, H, W), dev)
    lib.to_nchw(rows, off, c, back)
    run.cmp("to_nchw", "the round trip", back, x[:, c_begin:c_begin + c].double(), 0.0)
    run.sentinel("to_nchw", "images around the output", guards_of(whole))
    src = (torch.randn(B * N, 9, generator=gen)).to(dev)
    whole, o2 = guarded((B, 5, H, W), dev)
    lib.to_nchw(src, 3, 5, o2)
    run.cmp("to_nchw", "columns 3..8 of 9", o2, src[:, 3:8].double().view(B, H, W, 5).permute(0, 3, 1, 2), 0.0)
    run.sentinel("to_nchw", "images around the output", guards_of(whole))
    # pf_space_to_depth2: the 2H x 2W image whose output map is this shape's (H != W)
    for Cc in ((3, 1) if shape != "rows" else (3,)):
        Bs, Hs, Ws = (B, 2 * H, 2 * W) if shape != "rows" else ROWS_IMG
        xi = torch.randn(Bs, Cc, Hs, Ws, generator=gen).to(dev)
        ld_o = 4 * Cc + 3
        out = torch.full((Bs * (Hs // 2) * (Ws // 2), ld_o), SENT_F32, device=dev)
        lib.space_to_depth2(xi, out)
        run.cmp("space_to_depth2", f"C={Cc}", out[:, :4 * Cc], ref_s2d(xi), 0.0)
        run.sentinel("space_to_depth2", "columns past 4 C", out[:, 4 * Cc:])
    # pf_flow_prep: flow = coords1 - coords0, one fp32 subtraction: exact against torch's
    Bf, Hf, Wf = dims(shape)
    co = gc.nasty_coords(f"io/fp/{shape}", min(Bf, 2), Hf, Wf) if shape != "rows" else torch.rand(Bf, 2, Hf, Wf, generator=gen) * 3000 - 500
    co = co.to(dev)
    Bf = co.shape[0]
    ys, xs = torch.meshgrid(torch.arange(Hf, dtype=torch.float32, device=dev), torch.arange(Wf, dtype=torch.float32, device=dev), indexing="ij")
    want = (co - torch.stack([xs, ys])[None]).double()
    want_rows = want.permute(0, 2, 3, 1).reshape(-1, 2)
    for use in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
        wf, flow = guarded((Bf, 2, Hf, Wf), dev)
        d0 = torch.full((Bf * Hf * Wf, 7), SENT_F32, device=dev)
        d1 = torch.full((Bf * Hf * Wf, 5), SENT_F32, device=dev)
        lib.flow_prep(co, flow if use[0] else None, d0 if use[1] else None, 3, d1 if use[2] else None, 2)
        if use[0]:
            run.cmp("flow_prep", f"planar {use}", flow, want, 0.0)
        if use[1]:
            run.cmp("flow_prep", f"dst0 {use}", d0[:, 3:5], want_rows, 0.0)
        if use[2]:
            run.cmp("flow_prep", f"dst1 {use}", d1[:, 2:4], want_rows, 0.0)
        rest = [guards_of(wf), d0[:, :3].reshape(-1), d0[:, 5:].reshape(-1), d1[:, :2].reshape(-1), d1[:, 4:].reshape(-1)]
        rest += [t.reshape(-1) for t, u_ in ((flow, use[0]), (d0, use[1]), (d1, use[2])) if not u_]
        run.sentinel("flow_prep", f"everything not asked for {use}", torch.cat(rest))


# ------------------------------------------------------------------------------------------------------------------------
# family: relu  (pf_add_relu, pf_relu_mask)
# ------------------------------------------------------------------------------------------------------------------------
RELU_N = OrderedDict(n1=1, n1027=1027, rows=LOOP + 1027)


def run_relu(lib, shape, dev, run):
    """pf_add_relu is `v = x + y; v > 0 ? v : 0`: a NaN sum gives +0 (torch.relu would pass the NaN on), -0.0 gives +0.
    pf_relu_mask is `out > 0 ? g : 0` on the forward output: out = NaN or -0.0 masks the gradient to +0; a NaN gradient under an
    open mask passes as it is."""
    n = RELU_N[shape]
    gen = torch.Generator().manual_seed(91)
    x, y, g = (torch.randn(n, generator=gen) for _ in range(3))
    sx = torch.tensor([-0.0, float("nan"), 1.0, -0.0, 0.0, float("inf"), 2.0])
    sy = torch.tensor([0.0, 1.0, float("nan"), -0.0, -0.0, float("-inf"), -2.0])
    k = min(n, len(sx))
    x[n - k:], y[n - k:] = sx[:k], sy[:k]               # the specials sit in the ragged tail (n % 4 != 0)
    x, y, g = x.to(dev), y.to(dev), g.to(dev)
    whole = torch.full((n + 8,), SENT_F32, device=dev)
    out = whole[4:-4]
    lib.add_relu(x, y, out)
    v = x + y
    same_bits(run, "add_relu", "relu(x + y)", out, torch.where(v > 0, v, torch.zeros_like(v)))
    run.sentinel("add_relu", "floats around the output", torch.cat([whole[:4], whole[-4:]]))
    fwd = out.clone()
    fwd[:k] = torch.tensor([-0.0, float("nan"), 3.0, 0.0, 1e-40, -1.0, 5.0])[:k].to(dev)
    if n > 2:
        g[2] = float("nan")
    whole = torch.full((n + 8,), SENT_F32, device=dev)
    dx = whole[4:-4]
    lib.relu_mask(g, fwd, dx)
    same_bits(run, "relu_mask", "g where out > 0", dx, torch.where(fwd > 0, g, torch.zeros_like(g)))
    run.sentinel("relu_mask", "floats around the output", torch.cat([whole[:4], whole[-4:]]))


# ------------------------------------------------------------------------------------------------------------------------
# the case table
# ------------------------------------------------------------------------------------------------------------------------
IMG_SHAPES = ("even", "ragged", "w4", "eval", "rows")
FAMILIES = OrderedDict(
    grid=(run_grid, ("even", "ragged", "eval", "rows"), ("sample_grid",)),
    rotate=(run_rotate, IMG_SHAPES, ("img_rotate",)),
    prepare=(run_prepare, ("even", "ragged", "w4", "h8w28", "rows"), ("normalise_images", "prepare_images", "prepare_frame")),
    metrics=(run_metrics, ("eval", "ragged", "even", "rows"), ("flow_metrics_epe", "flow_metrics_hav", "flow_metrics_cos")),
    region=(run_region, ("ragged", "eval", "rows"), ("region_sums",)),
    pack=(run_pack, ("shapes", "rows"), ("pack_conv_weights",)),
    pack_batch=(run_pack_batch, ("jobs35",), ("pack_conv_weights_batch",)),
    unpack=(run_unpack, ("jobs35", "rows"), ("unpack_wgrads",)),
    layout=(run_layout, ("ragged", "rows"), ("to_channel_last", "to_nchw", "space_to_depth2", "flow_prep")),
    relu=(run_relu, tuple(RELU_N), ("add_relu", "relu_mask")),
)
CASES = [(fam, shape) for fam, (_, shapes, _) in FAMILIES.items() for shape in shapes]


def cases(device_type):
    return list(CASES)


def run_case(lib, family, shape, dev, table):
    """Runs one (family, shape) case; returns the list of failures (empty = pass).  A kernel of the family that left no row in
    the table at this shape is a failure of the case."""
    run = Run(table, shape)
    FAMILIES[family][0](lib, shape, dev, run)
    run.fails += [f"{k} [{shape}]: not in the table" for k in FAMILIES[family][2] if (k, shape) not in table.rows]
    return run.fails
