"""Launch-level checks of the gather, scatter, pointwise and reduction kernels against float64 (not a conftest, nothing here
is collected).  The same cases run on the CPU against the host emulation of csrc/pf_elem.h (tests/test_elem_launch_reference.py)
and on the GPU against the HIP library (tests/test_hip_elem_launches.py): one family of launches per case, every launch compared
element by element with a float64 torch statement of the same formula on the SAME fp32 inputs upcast, under a bound derived
below per output element.  Each launch is checked on its own inputs (a combine reads random rows, not the lookup's output), so a
bound never has to be propagated from one launch into the next; inside one kernel (the cross view of the lookup) it is.

Notation: U = 2^-24 (half an ulp of 1 in fp32; one rounding of a value v costs at most U |v|).

Bilinear gathers  v = sum_j w_j x_j  (pf_taps0 / pf_taps0v: zero padded, the four weights from one fp32 coordinate pair)
  * coordinate error.  A level coordinate c / 2^l + r is one rounding, U |c_l|.  pf_pymod is exact for 0 <= a < b and for
    |a| >= b (the remainder lies on a's grid), and one rounding of magnitude <= b otherwise: U W_l.  pf_roundtrip (pixel ->
    [-1, 1] -> pixel) is four roundings: 2p/s (U |p|), pn - 1 (U max(|p|, s/2)), pn + 1 (U (|p| + s)), the product (U |p|):
    RT(p, size) = U (4 |p| + 1.5 size).  dx, dy below are the sums of these for the kernel in question.
  * a coordinate error moves v by at most dx Dx + dy Dy, where Dx = max(|x01 - x00|, |x11 - x10|), Dy = max(|x10 - x00|,
    |x11 - x01|) are the differences over the sample's own cell of the zero-extended map (d v / d x is a convex combination of
    the two horizontal differences).  Zero-padded bilinear interpolation is continuous, but within dx (dy) of an integer the
    perturbed sample may use the neighbouring cell, whose values the cell differences do not see: there Dx = Dy = 2 max |map|
    (any difference of two values of the zero-extended map).
  * the seam.  The own view wraps x mod W_l and then zero-pads, so the sample jumps from ~0 (x -> W_l from below) to map[.., 0]
    (x = 0).  Rounding is monotone and k W_l is representable, so the fp32 coordinate crosses a multiple of W_l only by landing
    ON it from below: where W_l - x <= U |c_l| the bound gets 2 max |map|.  In the cross view x comes out of a gather with a
    two-sided error e, so the same term is added within e of either side of the seam.
  * fp32 roundings of the weights and the sum: 1 - w (1), the product of two factors (1), times the value (1), three additions
    (3), with the slack of one for a fused multiply-add counted either way: M_BILIN = 8, i.e. 8 U sum_j |w_j x_j|.
  * chained inside the lookup: the grid sample (gx, gy) carries its bound into dx, dy of the sample of the other pyramid.

Scatters with atomics  cell += sum over contributions c = w_j g
  * each weight is a product of two factors in [0, 1], each 1-Lipschitz in its coordinate: |dw_j| <= dx + dy, so a contribution
    is off by |g| (dx + dy) + 4 U |c| (weight roundings and the product), charged to the cell it lands in;
  * a contribution within dx, dy of an integer coordinate (or of the seam) may land in a neighbouring cell instead: its budget
    |g| (dx + dy) (the whole |g| at the seam) is charged to every cell of the 4 x 4 neighbourhood, cyclic in x;
  * unordered fp32 additions of n contributions onto an initial value g0: (n + 1) U (|g0| + sum |c|); the reference counts n
    and sums |c| per cell.  Two launches into the same buffer double the contributions.

Pointwise (GRU gate backward, frozen BatchNorm, norm_act, norm_bwd's apply pass, AdamW, pyramid_bwd): U times the magnitudes
entering each rounding, counted per formula next to the reference.  No sigmoid / tanh is recomputed in the gate kernels (z, r, q
are inputs), so they need no transcendental allowance; sqrtf / division are taken as 2 U relative each.  The convex upsampling
and its backward recompute a softmax: expf of l - max gets the project's device allowance EPS_TRANS = 2^-20 (absolute, values
<= 1; tests/conv_launches.py) and so does the division.  A ReLU mask decided by an fp32 value xh within its own error of 0 may
flip: there the masked gradient |g| is added to the bound (and to the bound of every sum it enters).

Dot products (warp_gcorr's group means over C/4 channels, flow_head_out's 9 C terms): (K + 1) U sum |term| for K terms in any
order -- the worst case, which a sum of random signs stays far below (ratios of 0.002 to 0.05 are that, not slack in a constant).

flo_rotate / motion_prep: piecewise smooth; the jumps (pf_unwrap_m, the +-W/2 clip) are detected on the float64 values and
added where they can happen, see the comment above ref_flo_rotate.  An element on a detected jump is off by nothing or by the
whole jump, so a worst ratio of 1.000 for these two kernels is such an element (about 0.1 % of them), not a bound that is met.
motion_prep's second warp samples at a computed point: the rotation's bound enters it as a coordinate error.

Reductions with fp64 partials (channel_stats, norm_bwd / bn_frozen_bwd sums, seq_loss, sum_squares): the per-term fp32
arithmetic (U per rounding, summed), the fp64 accumulation n 2^-53 sum |term|, and the final fp32 rounding U |result|.  Inputs
have per-channel variance of order 1 so that ss/N - mean^2 does not cancel.

AdamW: the per-step bound is applied at each of 3 steps, every step's reference starting from the state the launch started from;
pf_adamw_step_dev, fed the four scalars pf_adamw_step derives, is held to the same reference and bound.

Exact entries (sentinel rows and columns, pf_coords_add, the clear_raw zeroes, loss gradients' signs) have bound 0.
"""
import math
from collections import OrderedDict

import numpy as np
import torch

import golden_cases as gc
import priorflow_oracle as po        # input grids only; the arithmetic under test is restated below

U = 2.0 ** -24
U64 = 2.0 ** -53
M_BILIN = 8
SENT_F32 = -1234.5                   # sentinel of every column / row a launch must not write (as tests/conv_launches.py)
CORR_LEVELS, CORR_RADIUS, TAPS, CORR_CH = 4, 4, 81, 324

# csrc/pf_elem_kernels.hip: `constexpr long kMaxBlocks = 256L * 64` blocks per launch, grid-stride beyond that.  The wave-per-row
# kernels (pf_lookup_bwd_rows, pf_upsample_bwd_wave) take 4 rows per block, so a wave walks a second row only beyond
# 4 * K_MAX_BLOCKS = 65536 rows; the 256-thread elementwise kernels loop beyond 256 * K_MAX_BLOCKS = 4.2 M elements.
K_MAX_BLOCKS = 256 * 64
ROWS_B = 4 * K_MAX_BLOCKS // 256 + 4      # 260 images of 16 x 16: one pass of the row kernels (65 536 rows) and 1 024 rows more
SHAPES = OrderedDict(even=(2, 16, 32), ragged=(3, 17, 27), folded=(1, 16, 16), rows=(ROWS_B, 16, 16))
ROW_COUNTS = OrderedDict(one=1, some=200, rows=ROWS_B * 256)          # row-matrix kernels (GRU gates, norm, BN)
# (B, Np, nblk) of the per-(image, channel) statistics and the kernels around them: the reduction edges (empty chunks, a ragged last
# chunk, 7 chunks, nblk == Np) and the row counts 1 / 200 / 66 560 of the row-matrix kernels (the last with the product's nblk)
STAT_SHAPES = OrderedDict(empty=(2, 64, 128), ragged=(2, 459, 128), seven=(2, 240, 7), full=(2, 96, 96),
                          one=(1, 1, 1), some=(2, 100, 16), rows=(ROWS_B, 256, 128))


# ------------------------------------------------------------------------------------------------------------------------
# the table and the checker
# ------------------------------------------------------------------------------------------------------------------------
class Table:
    """worst |err| / bound per (kernel, shape)."""

    def __init__(self):
        self.rows = OrderedDict()

    def add(self, kernel, shape, r):
        key = (kernel, shape)
        self.rows[key] = max(self.rows.get(key, 0.0), r)

    def render(self):
        out = [f"{'kernel':<28} {'shape':<10} worst |err|/bound"]
        out += [f"{k:<28} {s:<10} {r:.3f}" for (k, s), r in self.rows.items()]
        return "\n".join(out)

    def per_kernel(self):
        d = OrderedDict()
        for (k, _), r in self.rows.items():
            d[k] = max(d.get(k, 0.0), r)
        return d


def ratio(got, ref, bound):
    """max |got - ref| / bound; an element with bound 0 must be equal (inf otherwise); non-finite output is inf."""
    got = got.double()
    if got.shape != ref.shape:
        raise AssertionError(("shape", tuple(got.shape), tuple(ref.shape)))
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    err = (got - ref).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64, device=err.device).expand_as(err)
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)       # 0/0 -> 0, x/0 -> inf
    return float(r.max()) if r.numel() else 0.0


class Run:
    """One case's bookkeeping: outputs compared, sentinels checked, failures collected."""

    def __init__(self, table, shape):
        self.table, self.shape, self.fails = table, shape, []

    def cmp(self, kernel, what, got, ref, bound):
        r = ratio(got, ref, bound)
        self.table.add(kernel, self.shape, r)
        if not r <= 1.0:
            self.fails.append(f"{kernel} [{self.shape}] {what}: |err|/bound = {r:.3g}")
        return r

    def sentinel(self, kernel, what, t):
        if t.numel() and not bool((t == SENT_F32).all()):
            self.fails.append(f"{kernel} [{self.shape}] {what}: a sentinel was overwritten")
            self.table.add(kernel, self.shape, float("inf"))


def widths_of(shape_name):
    """The model's channel widths of the row-matrix kernels; a shape named `<shape>_c<width>` is the sibling of <shape> at that
    one width (what the CPU runs where the full case is too slow for a unit test there)."""
    return (int(shape_name.split("_c")[1]),) if "_c" in shape_name else (64, 96, 128)


def rnd(gen, shape, lo, hi, dev):
    return (torch.rand(shape, generator=gen) * (hi - lo) + lo).to(dev)


def padded(t, ld, col=0):
    """fp32 rows [R, C] inside a sentinel matrix [R, ld] at column `col`: (whole, view)."""
    whole = torch.full((t.shape[0], ld), SENT_F32, device=t.device)
    whole[:, col:col + t.shape[1]] = t
    return whole, whole[:, col:col + t.shape[1]]


def padded_unaligned(t, ld):
    """As `padded`, but the matrix starts one float into its allocation: contiguous rows whose base is not 16-byte aligned."""
    flat = torch.full((t.shape[0] * ld + 1,), SENT_F32, device=t.device)
    whole = flat[1:].view(t.shape[0], ld)
    whole[:, :t.shape[1]] = t
    assert whole.is_contiguous() and whole.data_ptr() % 16 == 4
    return whole, flat[:1]


def outside(whole, col, width):
    return torch.cat([whole[:, :col], whole[:, col + width:]], 1)


# ------------------------------------------------------------------------------------------------------------------------
# bilinear taps in float64
# ------------------------------------------------------------------------------------------------------------------------
def last_chunk_start(n, nblk):
    """First element of the last non-empty chunk of the kernels' `chunk = ceil(n / nblk)` split."""
    chunk = -(-n // nblk)
    return ((n - 1) // chunk) * chunk


def rt_err(p, size):
    return U * (4.0 * p.abs() + 1.5 * size)


def taps0(Hl, Wl, x, y, mut=None):
    """The four zero-padded taps of pf_taps0 at pixel coordinates (x, y) of an Hl x Wl map: [(idx, w, ok)] in the order
    nw, ne, sw, se, and the fractions.  mut == 'drop_tap' loses the fourth."""
    fx, fy = torch.floor(x), torch.floor(y)
    wx, wy = x - fx, y - fy
    out = []
    for ox, oy in ((0, 0), (1, 0), (0, 1), (1, 1)):
        xi, yi = fx + ox, fy + oy
        ok = (xi >= 0) & (xi <= Wl - 1) & (yi >= 0) & (yi <= Hl - 1)
        w = (wx if ox else 1.0 - wx) * (wy if oy else 1.0 - wy)
        w = torch.where(ok, w, torch.zeros_like(w))
        idx = (yi.clamp(0, Hl - 1) * Wl + xi.clamp(0, Wl - 1)).long()
        out.append((idx, w, ok))
    if mut == "drop_tap":
        out[3] = (out[3][0], torch.zeros_like(out[3][1]), out[3][2])
    return out, (fx, fy, wx, wy)


def bilin0(maps, Hl, Wl, x, y, dx, dy, mut=None):
    """maps [R or 1, Hl*Wl] float64, x / y [R, K] float64 (x already wrapped), dx / dy coordinate error bounds -> value, bound."""
    taps, (_, _, wx, wy) = taps0(Hl, Wl, x, y, mut)
    if maps.shape[0] == 1 and x.shape[0] != 1:
        maps = maps.expand(x.shape[0], -1)
    vals = [torch.gather(maps, 1, idx) * ok for idx, _, ok in taps]
    v = sum(val * w for val, (_, w, _) in zip(vals, taps))
    absw = sum((val * w).abs() for val, (_, w, _) in zip(vals, taps))
    Dx = torch.maximum((vals[1] - vals[0]).abs(), (vals[3] - vals[2]).abs())
    Dy = torch.maximum((vals[2] - vals[0]).abs(), (vals[3] - vals[1]).abs())
    L = 2.0 * maps.abs().amax(1, keepdim=True)
    near = (torch.minimum(wx, 1.0 - wx) <= dx) | (torch.minimum(wy, 1.0 - wy) <= dy)
    Dx, Dy = torch.where(near, L.expand_as(Dx), Dx), torch.where(near, L.expand_as(Dy), Dy)
    return v, dx * Dx + dy * Dy + M_BILIN * U * absw, L


def edge_coords(tag, B, H, W, gen):
    """gc.nasty_coords (rows 0-5: integers, the seam fade, x = -0.25, y half out, far below, 2.5 wraps) and, below them, the
    edge list of test_hip_kernels._lookup_window_case: exact integers, multi-wrap and negative x, y far outside, x in (W-1, W)
    and on W, flows of +-W/2."""
    co = gc.nasty_coords(tag, min(B, 4), H, W)
    co = co.repeat((B + co.shape[0] - 1) // co.shape[0], 1, 1, 1)[:B].clone()
    base = torch.stack(torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")[::-1])
    flow = (torch.rand(B, 2, H, W, generator=gen) - 0.5) * 24.0
    flow[:, :, ::3, ::5] = torch.round(flow[:, :, ::3, ::5])
    flow[:, 0, 1::4] += 2.5 * W
    flow[:, 0, 2::4] -= 1.75 * W
    flow[:, 1, :, 3::7] += 3.0 * H
    flow[:, 1, :, 5::7] -= 2.0 * H
    flow[:, :, 6] = 0.0
    flow[:, 0, 6, ::2] = W / 2.0
    flow[:, 0, 6, 1::2] = -W / 2.0
    w = (base[None] + flow)
    co[:, :, 6:] = w[:, :, 6:]
    co[:, 0, 7, :4] = torch.tensor([W - 0.5, W - 1.0, -0.25, W + 0.0])
    return co.contiguous()


def grids(H, W, kind, gen, theta):
    if kind == "real":
        return po.sample_grid(H, W, po.rotation_x(theta)).contiguous()
    return torch.stack([torch.rand(H, W, generator=gen) * (W + 4) - 2, torch.rand(H, W, generator=gen) * (H + 4) - 2]).contiguous()


def level_dims(H, W, lvl, mut=None):
    if mut == "ceil_width":
        return H >> lvl, -(-W // (1 << lvl))
    return H >> lvl, W >> lvl


def lookup_geometry(coords, grid, H, W, lvl, mut=None):
    """Coordinates and their error bounds of level `lvl` of pf_lookup_elem / pf_lookup_bwd_elem for rows [R] of coords [R, 2]
    (float64): the own-view sample (xo, cy, dx, dy, seam) and a closure for the cross view."""
    Hl, Wl = level_dims(H, W, lvl, mut)
    inv = 0.5 ** lvl
    r = torch.arange(9, dtype=torch.float64, device=coords.device) - (CORR_RADIUS if mut != "origin_off" else CORR_RADIUS - 1)
    off_x = r.view(9, 1).expand(9, 9).reshape(1, TAPS)          # the slow window axis offsets x (core/corr.py:120-126)
    off_y = r.view(1, 9).expand(9, 9).reshape(1, TAPS)
    cx = coords[:, 0:1] * inv + off_x
    cy = coords[:, 1:2] * inv + off_y
    e_cx, e_cy = U * cx.abs(), U * cy.abs()
    wrap_w = Wl if mut != "seam_off" else Wl - 1
    xo = torch.remainder(cx, wrap_w)
    own = dict(x=xo, y=cy, dx=e_cx + U * Wl + rt_err(xo, Wl), dy=e_cy + rt_err(cy, Hl), seam=(Wl - xo) <= e_cx)
    xg = torch.remainder(cx, W)
    dxg, dyg = e_cx + U * W + rt_err(xg, W), e_cy + rt_err(cy, H)
    N = H * W
    gx, bgx, Lx = bilin0(grid[0].reshape(1, N), H, W, xg, cy, dxg, dyg)
    gy, bgy, Ly = bilin0(grid[1].reshape(1, N), H, W, xg, cy, dxg, dyg)
    seam_g = (W - xg) <= e_cx
    bgx, bgy = bgx + seam_g * Lx, bgy + seam_g * Ly
    xw = torch.remainder(gx, wrap_w)
    oth = dict(x=xw, y=gy, dx=bgx + U * Wl + rt_err(xw, Wl), dy=bgy + rt_err(gy, Hl), seam=((Wl - xw) <= bgx) | (xw <= bgx))
    return Hl, Wl, own, oth


# ------------------------------------------------------------------------------------------------------------------------
# family: lookup  (dccl_lookup planar / interleaved grid, dccl_combine)
# ------------------------------------------------------------------------------------------------------------------------
def lookup_case(shape, dev, grid_kind="real", seed=1):
    B, H, W = SHAPES[shape]
    R = B * H * W
    gen = torch.Generator().manual_seed(seed)
    c = dict(shape=shape, B=B, H=H, W=W, R=R)
    c["coords"] = edge_coords(f"el/{shape}", B, H, W, gen).to(dev)
    c["grid"] = grids(H, W, grid_kind, gen, math.pi / 2).to(dev)
    c["g_back"] = grids(H, W, grid_kind, gen, -math.pi / 2).to(dev)
    c["own"] = [rnd(gen, (R, (H >> l) * (W >> l)), -4, 4, dev) for l in range(CORR_LEVELS)]
    c["oth"] = [rnd(gen, (R, (H >> l) * (W >> l)), -4, 4, dev) for l in range(CORR_LEVELS)]
    return c


def _rows_of(coords):
    B, _, H, W = coords.shape
    return coords.double().permute(0, 2, 3, 1).reshape(B * H * W, 2)


def ref_lookup(c, mut=None, chunk=8192):
    """own / raw [R, 324] float64 and their bounds."""
    H, W, R = c["H"], c["W"], c["R"]
    co = _rows_of(c["coords"])
    grid = c["grid"].double()
    outs = [torch.empty(R, CORR_CH, dtype=torch.float64, device=co.device) for _ in range(4)]
    for lvl in range(CORR_LEVELS):
        for r0 in range(0, R, chunk):
            sl = slice(r0, min(R, r0 + chunk))
            Hl, Wl, o, x = lookup_geometry(co[sl], grid, H, W, lvl, mut)
            res = []
            for g, maps in ((o, c["own"][lvl]), (x, c["oth"][lvl])):
                m = maps[sl].double()
                if mut == "ceil_width":               # the (wrong) wider rows index past the map: pad it
                    m = torch.cat([m, torch.zeros(m.shape[0], Hl * Wl - m.shape[1], dtype=m.dtype, device=m.device)], 1)
                v, b, L = bilin0(m, Hl, Wl, g["x"], g["y"], g["dx"], g["dy"], mut)
                res += [v, b + g["seam"] * L]
            for t, v in zip(outs, res):
                t[sl, lvl * TAPS:(lvl + 1) * TAPS] = v
    return dict(own=(outs[0], outs[1]), raw=(outs[2], outs[3]))


def run_lookup(lib, c, run, refs=None):
    R, H, W = c["R"], c["H"], c["W"]
    refs = refs or ref_lookup(c)
    dev = c["coords"].device
    g_il = c["grid"].reshape(2, -1).t().contiguous()
    for kernel, ld, il in (("dccl_lookup", 336, None), ("dccl_lookup_il", 325, g_il)):
        own = torch.full((R, ld), SENT_F32, device=dev)
        raw = torch.full((R, ld), SENT_F32, device=dev)
        lib.dccl_lookup(c["coords"], c["own"], c["oth"], c["grid"], own, raw, il)
        run.cmp(kernel, "own", own[:, :CORR_CH], *refs["own"])
        run.cmp(kernel, "raw", raw[:, :CORR_CH], *refs["raw"])
        run.sentinel(kernel, "own padding", own[:, CORR_CH:])
        run.sentinel(kernel, "raw padding", raw[:, CORR_CH:])


def combine_case(shape, dev, grid_kind="real", seed=2):
    B, H, W = SHAPES[shape]
    R = B * H * W
    gen = torch.Generator().manual_seed(seed)
    c = dict(shape=shape, B=B, H=H, W=W, R=R)
    c["g_back"] = grids(H, W, grid_kind, gen, -math.pi / 2).to(dev)
    c["own"] = rnd(gen, (R, CORR_CH), -3, 3, dev)
    c["raw"] = rnd(gen, (R, CORR_CH), -3, 3, dev)
    c["d_corr"] = rnd(gen, (R, CORR_CH), -1, 1, dev)
    c["d_raw0"] = rnd(gen, (R, CORR_CH), -1, 1, dev)
    return c


def combine_geometry(c, mut=None):
    H, W = c["H"], c["W"]
    g = c["g_back"].double().reshape(2, 1, H * W)
    x = torch.remainder(g[0], W)
    y = g[1]
    dx, dy = U * W + rt_err(x, W), rt_err(y, H)
    return x, y, dx, dy


def ref_combine(c, mut=None, chunk=16):
    B, H, W = c["B"], c["H"], c["W"]
    N = H * W
    x, y, dx, dy = combine_geometry(c, mut)
    out = torch.empty(c["R"], CORR_CH, dtype=torch.float64, device=x.device)
    bnd = torch.empty_like(out)
    own, raw = c["own"].double().view(B, N, CORR_CH), c["raw"].double().view(B, N, CORR_CH)
    for b0 in range(0, B, chunk):
        m = raw[b0:b0 + chunk].permute(0, 2, 1).reshape(-1, N)                 # [(b, k), N]
        e = lambda t: t.expand(m.shape[0], N)                                  # noqa: E731
        v, bv, _ = bilin0(m, H, W, e(x), e(y), e(dx), e(dy), mut)
        nb = m.shape[0] // CORR_CH
        v = v.view(nb, CORR_CH, N).permute(0, 2, 1)
        o = own[b0:b0 + chunk] + v
        out.view(B, N, CORR_CH)[b0:b0 + chunk] = o
        bnd.view(B, N, CORR_CH)[b0:b0 + chunk] = bv.view(nb, CORR_CH, N).permute(0, 2, 1) + U * o.abs()
    return dict(out=(out, bnd))


def ref_combine_bwd(c, launches=1):
    B, H, W = c["B"], c["H"], c["W"]
    N = H * W
    x, y, dx, dy = combine_geometry(c)
    S, E, Cn = (m[0] for m in scatter_mats(H, W, x, y, dx, dy, torch.zeros_like(x, dtype=torch.bool)))      # one grid for the batch
    g = c["d_corr"].double().view(B, N, CORR_CH)
    d0 = c["d_raw0"].double().view(B, N, CORR_CH)
    add = torch.matmul(S, g)
    A = torch.matmul(S, g.abs())
    n = Cn.sum(1).view(1, N, 1)
    ref = d0 + launches * add
    bnd = launches * (torch.matmul(E, g.abs()) + 4 * U * A) + (launches * n + 1) * U * (d0.abs() + launches * A)
    return dict(d_raw=(ref.reshape(-1, CORR_CH), bnd.reshape(-1, CORR_CH)))


def run_combine(lib, c, run):
    B, H, W, R = c["B"], c["H"], c["W"], c["R"]
    ref = ref_combine(c)
    for ld, ld_out in ((336, 336), (336, 325), (325, 336)):  # launch_combine picks vector or scalar code from both ld % 4
        own, _ = padded(c["own"], ld)
        raw, _ = padded(c["raw"], ld)
        out = torch.full((R, ld_out), SENT_F32, device=own.device)
        lib.dccl_combine(own, raw, c["g_back"], out, B, H, W)
        run.cmp("dccl_combine", f"out ld={ld}->{ld_out}", out[:, :CORR_CH], *ref["out"])
        run.sentinel("dccl_combine", "out padding", out[:, CORR_CH:])
    # ld % 4 == 0 everywhere but a base 4 bytes off a 16-byte boundary: launch_combine must take the scalar statement
    (own, h0), (raw, h1), (out, h2) = (padded_unaligned(t, 336) for t in (c["own"], c["raw"], torch.full_like(c["own"], SENT_F32)))
    lib.dccl_combine(own, raw, c["g_back"], out, B, H, W)
    run.cmp("dccl_combine", "out, unaligned bases", out[:, :CORR_CH], *ref["out"])
    run.sentinel("dccl_combine", "out padding and the float before it", torch.cat([out[:, CORR_CH:].reshape(-1), h0, h1, h2]))
    refb = ref_combine_bwd(c)
    for ld_in, ld in ((336, 336), (336, 325), (325, 336)):
        d_corr, _ = padded(c["d_corr"], ld_in)
        d_raw, _ = padded(c["d_raw0"], ld)
        lib.dccl_combine_bwd(d_corr, c["g_back"], d_raw, B, H, W)
        run.cmp("dccl_combine_bwd", f"d_raw ld={ld_in}->{ld}", d_raw[:, :CORR_CH], *refb["d_raw"])
        run.sentinel("dccl_combine_bwd", "d_raw padding", d_raw[:, CORR_CH:])


# ------------------------------------------------------------------------------------------------------------------------
# family: lookup_bwd  (dccl_lookup_bwd, clear_raw off then on, two launches into the same gradients)
# ------------------------------------------------------------------------------------------------------------------------
def lookup_bwd_case(shape, dev, grid_kind="real", seed=3):
    c = lookup_case(shape, dev, grid_kind, seed)
    gen = torch.Generator().manual_seed(seed + 100)
    R, H, W = c["R"], c["H"], c["W"]
    c["d_own"] = rnd(gen, (R, CORR_CH), -1, 1, dev)
    c["d_raw"] = rnd(gen, (R, CORR_CH), -1, 1, dev)
    c["g_own0"] = [rnd(gen, (R, (H >> l) * (W >> l)), -1, 1, dev) for l in range(CORR_LEVELS)]
    c["g_oth0"] = [rnd(gen, (R, (H >> l) * (W >> l)), -1, 1, dev) for l in range(CORR_LEVELS)]
    del c["own"], c["oth"]
    return c


def _scatter_level(g, geo, Hl, Wl, g0, launches, mut=None):
    """One level, one view: g [R, 81] upstream gradients, geo the sample geometry -> (reference, bound) [R, Hl*Wl]."""
    R, lsz = g.shape[0], Hl * Wl
    taps, (fx, fy, wx, wy) = taps0(Hl, Wl, geo["x"], geo["y"], mut)
    z = lambda: torch.zeros(R, lsz, dtype=torch.float64, device=g.device)       # noqa: E731
    add, A, E, n = z(), z(), z(), z()
    dxy = geo["dx"] + geo["dy"]
    for idx, w, ok in taps:
        add.scatter_add_(1, idx, w * g)
        A.scatter_add_(1, idx, (w * g).abs())
        E.scatter_add_(1, idx, g.abs() * dxy * ok)
        n.scatter_add_(1, idx, (w != 0).double())
    near = (torch.minimum(wx, 1.0 - wx) <= geo["dx"]) | (torch.minimum(wy, 1.0 - wy) <= geo["dy"]) | geo["seam"]
    rr, kk = torch.nonzero(near, as_tuple=True)
    if rr.numel():
        budget = (g.abs() * torch.where(geo["seam"], torch.ones_like(dxy), dxy))[rr, kk]
        bx, by = fx[rr, kk], fy[rr, kk]
        flat = E.view(-1)
        for oy in (-1, 0, 1, 2):
            yy = by + oy
            oky = (yy >= 0) & (yy <= Hl - 1)
            for ox in (-1, 0, 1, 2):
                xx = torch.remainder(bx + ox, Wl)
                cell = rr * lsz + (yy.clamp(0, Hl - 1) * Wl + xx).long()
                flat.index_put_((cell,), budget * oky, accumulate=True)
    if mut == "lose_second":
        launches = 1
    ref = g0 + launches * add
    bnd = launches * (E + 4 * U * A) + (launches * n + 1) * U * (g0.abs() + launches * A)
    return ref, bnd


def ref_lookup_bwd(c, launches=2, mut=None, chunk=8192):
    H, W, R = c["H"], c["W"], c["R"]
    co = _rows_of(c["coords"])
    grid = c["grid"].double()
    out = {}
    for lvl in range(CORR_LEVELS):
        lsz = (H >> lvl) * (W >> lvl)
        refs = [torch.empty(R, lsz, dtype=torch.float64, device=co.device) for _ in range(4)]
        for r0 in range(0, R, chunk):
            sl = slice(r0, min(R, r0 + chunk))
            Hl, Wl, o, x = lookup_geometry(co[sl], grid, H, W, lvl)
            ks = slice(lvl * TAPS, (lvl + 1) * TAPS)
            refs[0][sl], refs[1][sl] = _scatter_level(c["d_own"][sl, ks].double(), o, Hl, Wl, c["g_own0"][lvl][sl].double(), launches, mut)
            refs[2][sl], refs[3][sl] = _scatter_level(c["d_raw"][sl, ks].double(), x, Hl, Wl, c["g_oth0"][lvl][sl].double(), launches, mut)
        out[f"g_own{lvl}"] = (refs[0], refs[1])
        out[f"g_other{lvl}"] = (refs[2], refs[3])
    return out


def run_lookup_bwd(lib, c, run, ld=336, refs=None):
    refs = refs or ref_lookup_bwd(c)
    d_own, _ = padded(c["d_own"], ld)
    d_raw, _ = padded(c["d_raw"], ld)
    g_own = [t.clone() for t in c["g_own0"]]
    g_oth = [t.clone() for t in c["g_oth0"]]
    lib.dccl_lookup_bwd(c["coords"], c["grid"], d_own, d_raw, g_own, g_oth, clear_raw=False)
    if not torch.equal(d_raw[:, :CORR_CH], c["d_raw"]):
        run.fails.append(f"dccl_lookup_bwd [{run.shape}]: d_raw changed without clear_raw")
    lib.dccl_lookup_bwd(c["coords"], c["grid"], d_own, d_raw, g_own, g_oth, clear_raw=True)
    for lvl in range(CORR_LEVELS):
        run.cmp("dccl_lookup_bwd", f"own level {lvl}", g_own[lvl], *refs[f"g_own{lvl}"])
        run.cmp("dccl_lookup_bwd", f"other level {lvl}", g_oth[lvl], *refs[f"g_other{lvl}"])
    run.cmp("dccl_lookup_bwd", "clear_raw", d_raw[:, :CORR_CH], torch.zeros_like(c["d_raw"], dtype=torch.float64), 0.0)
    run.sentinel("dccl_lookup_bwd", "d_raw padding", d_raw[:, CORR_CH:])
    run.cmp("dccl_lookup_bwd", "d_own untouched", d_own[:, :CORR_CH], c["d_own"].double(), 0.0)
    return d_raw


# ------------------------------------------------------------------------------------------------------------------------
# family: pyramid_bwd, coords_add
# ------------------------------------------------------------------------------------------------------------------------
def ref_pyramid_bwd(g, H, W, mut=None):
    """dV = g0 + sum_i g_i[y >> i][x >> i] / 4^i where the parent exists at every level up to i; bound: one rounding per add."""
    R = g[0].shape[0]
    v = g[0].double().view(R, H, W).clone()
    mag = v.abs()
    ys = torch.arange(H, device=v.device).view(H, 1)
    xs = torch.arange(W, device=v.device).view(1, W)
    alive = torch.ones(H, W, dtype=torch.bool, device=v.device)
    for i in (1, 2, 3):
        hy, hx = H >> i, W >> i
        py, px = ys >> i, xs >> i
        alive = alive & (py < hy) & (px < hx)
        lv = g[i].double().view(R, hy, hx)
        term = lv[:, py.clamp(max=hy - 1).expand(H, W), px.clamp(max=hx - 1).expand(H, W)] * (0.25 ** i) * alive
        v = v + term
        mag = mag + term.abs()
    return v.view(R, H * W), 3 * U * mag.view(R, H * W)


def run_small(lib, shape, dev, run):
    B, H, W = SHAPES[shape]
    N, R = H * W, B * H * W
    gen = torch.Generator().manual_seed(11)
    # pyramid_bwd: a pf_launch_elem kernel over rows * H * W elements
    g = [rnd(gen, (R, (H >> l) * (W >> l)), -1, 1, dev) for l in range(CORR_LEVELS)]
    ref, bnd = ref_pyramid_bwd(g, H, W)
    keep = [t.clone() for t in g[1:]]
    lib.pyramid_bwd(g, B, H, W)
    run.cmp("pyramid_bwd", "dV", g[0], ref, bnd)
    for a, b in zip(keep, g[1:]):
        run.cmp("pyramid_bwd", "parents untouched", b, a.double(), 0.0)
    # coords_add, in place and src=: one fp32 addition, exact against fp32 torch
    co = edge_coords(f"el/ca/{shape}", B, H, W, gen).to(dev)
    for ld in (4, 5):
        delta = torch.full((R, ld), SENT_F32, device=dev)
        delta[:, :2] = rnd(gen, (R, 2), -1, 1, dev)
        want = (co + delta[:, :2].reshape(B, H, W, 2).permute(0, 3, 1, 2)).double()
        c1 = co.clone()
        lib.coords_add(c1, delta)
        run.cmp("coords_add", f"in place ld={ld}", c1, want, 0.0)
        c2 = torch.full_like(co, SENT_F32)
        lib.coords_add(c2, delta, src=co)
        run.cmp("coords_add_to", f"src= ld={ld}", c2, want, 0.0)
        run.sentinel("coords_add", "delta padding", delta[:, 2:])


# ------------------------------------------------------------------------------------------------------------------------
# family: gru  (gru_q_bwd, gru_zr_bwd, gru_dx_finish) -- row views with a column offset of 1 and ld 325 / 336
# ------------------------------------------------------------------------------------------------------------------------
def ref_gru_q(g, z, q, h, mut=None):
    zz = 1.0 - z if mut == "swap_z" else z
    dq = (g * zz) * (1.0 - q * q)
    dz = g * q - g * h
    dh = g * (1.0 - zz)
    return dict(dq_pre=(dq, 4 * U * (g * zz).abs() * (1.0 + q * q)),
                dz=(dz, 2 * U * ((g * q).abs() + (g * h).abs())),
                dh=(dh, 2 * U * g.abs() * (1.0 + zz.abs())))


def ref_gru_zr(dz, drh, z, r, h, dh0):
    a = (dz * (1.0 - z)) * z
    b = ((drh * h) * (1.0 - r)) * r
    dh = dh0 + drh * r
    return dict(dz_pre=(a, 3 * U * dz.abs() * (1.0 + z.abs()) * z.abs()),
                dr_pre=(b, 4 * U * (drh * h).abs() * (1.0 + r.abs()) * r.abs()),
                dh=(dh, 2 * U * (dh0.abs() + (drh * r).abs())))


def run_gru(lib, rows_name, dev, run):
    for Cc in widths_of(rows_name):
        _run_gru(lib, rows_name, dev, run, Cc)


def _run_gru(lib, rows_name, dev, run, Cc):
    rows = ROW_COUNTS[rows_name.split("_c")[0]]
    gen = torch.Generator().manual_seed(21 + rows + Cc)
    D = lambda t: t.double()                                                     # noqa: E731
    mk = lambda lo, hi, ld, col, w=Cc: padded(rnd(gen, (rows, w), lo, hi, dev), ld, col)     # noqa: E731
    # inputs sit at column 1 of rows of 325 floats (no 16-byte alignment anywhere) or at column 0 of 336
    (Wg, g), (Wz, z), (Wq, q), (Wh, h) = mk(-1, 1, 325, 1), mk(0.02, 0.98, 336, 0), mk(-0.98, 0.98, 325, 1), mk(-1, 1, Cc + 1, 1)
    wide = torch.full((rows, 3 * Cc + 2), SENT_F32, device=dev)
    dq, dz, dh = wide[:, 1:1 + Cc], wide[:, 1 + Cc:1 + 2 * Cc], wide[:, 1 + 2 * Cc:1 + 3 * Cc]
    lib.gru_q_bwd(g, z, q, h, dq, dz, dh)
    ref = ref_gru_q(D(g), D(z), D(q), D(h))
    for name, t in (("dq_pre", dq), ("dz", dz), ("dh", dh)):
        run.cmp("gru_q_bwd", name, t, *ref[name])
    run.sentinel("gru_q_bwd", "outer columns", wide[:, [0, 3 * Cc + 1]])
    (Wr, r), (Wd, drh) = mk(0.02, 0.98, 325, 1), mk(-1, 1, 336, 0)
    dh0 = dh.clone()
    dz_in = dz.clone().contiguous()
    dzr = torch.full((rows, 2 * Cc + 9), SENT_F32, device=dev)
    lib.gru_zr_bwd(dz_in, drh, z, r, h, dzr[:, 1:], dh)
    ref = ref_gru_zr(D(dz_in), D(drh), D(z), D(r), D(h), D(dh0))
    run.cmp("gru_zr_bwd", "dz_pre", dzr[:, 1:1 + Cc], *ref["dz_pre"])
    run.cmp("gru_zr_bwd", "dr_pre", dzr[:, 1 + Cc:1 + 2 * Cc], *ref["dr_pre"])
    run.cmp("gru_zr_bwd", "dh", dh, *ref["dh"])
    run.sentinel("gru_zr_bwd", "dzr padding", outside(dzr, 1, 2 * Cc))
    run.sentinel("gru_zr_bwd", "outer columns", wide[:, [0, 3 * Cc + 1]])
    for wout in (Cc - 4, Cc - 2):                            # 124 and 126 at the model's width
        wd = Cc + wout
        (F1, f1), (F2, f2), (X, x) = mk(-1, 1, wd + 3, 1, wd), mk(-1, 1, wd + 2, 0, wd), mk(-1, 1, wd + 7, 1, wd)
        x[:, Cc::5] = 0.0                                    # exactly zero is masked
        Di, d_inp = mk(-1, 1, Cc + 1, 1)
        d0 = d_inp.clone()
        Do = torch.full((rows, wout + 2), SENT_F32, device=dev)
        lib.gru_dx_finish(f1, f2, x, d_inp, Do[:, 1:1 + wout], Cc, wout)
        s = D(f1) + D(f2)
        run.cmp("gru_dx_finish", f"d_inp wout={wout}", d_inp, D(d0) + s[:, :Cc], 2 * U * (D(d0).abs() + D(f1)[:, :Cc].abs() + D(f2)[:, :Cc].abs()))
        keep = D(x)[:, Cc:] > 0
        run.cmp("gru_dx_finish", f"d_out wout={wout}", Do[:, 1:1 + wout], s[:, Cc:] * keep, U * s[:, Cc:].abs() * keep)
        run.sentinel("gru_dx_finish", "d_out outer columns", Do[:, [0, wout + 1]])
        run.sentinel("gru_dx_finish", "d_inp outer column", Di[:, :1])
    for whole, col in ((Wg, 1), (Wz, 0), (Wq, 1), (Wh, 1), (Wr, 1), (Wd, 0)):
        run.sentinel("gru_zr_bwd", "input padding", outside(whole, col, Cc))


# ------------------------------------------------------------------------------------------------------------------------
# family: norm  (channel_stats + norm_act in four forms, norm_bwd instance / fixed, with and without ReLU)
# ------------------------------------------------------------------------------------------------------------------------
EPS_NORM = float(np.float32(1e-5))


def ref_stats(y, B, Np, Cc, mut=None, nblk=None):
    """scale = rsqrt(var + eps), shift = -mean * scale from float64 sums (biased variance); only the final fp32 rounding, the
    fp64 accumulation of Np terms and the conditioning of ss/N - mean^2 (|mean|^2 + var against var + eps) contribute."""
    v = y.double().view(B, Np, Cc)
    if mut == "drop_chunk":
        v = v[:, :last_chunk_start(Np, nblk)]
        mean, ex2 = v.sum(1) / Np, (v * v).sum(1) / Np
        var = ex2 - mean * mean
    else:
        mean = v.mean(1)
        var = ((v - mean[:, None]) ** 2).mean(1)
    if mut == "unbiased":
        var = var * Np / (Np - 1)
    rstd = 1.0 / torch.sqrt(var + EPS_NORM)
    cond = Np * U64 * ((v * v).mean(1) + mean * mean) / (var + EPS_NORM)       # relative effect of the fp64 sums on rstd
    sc, sh = rstd, -mean * rstd
    return dict(scale=(sc, (U + cond) * sc.abs()), shift=(sh, (U + cond) * sh.abs() + Np * U64 * v.abs().mean(1) * rstd))


def ref_norm_act(y, s, t, B, Np, Cc, res=None, rs=None, rt=None, res_relu=False):
    e = lambda p: p.double().view(B, 1, Cc)                                      # noqa: E731
    yv = y.double().view(B, Np, Cc)
    a = yv * e(s) + e(t)
    v = a.clamp_min(0)
    bnd = 2 * U * ((yv * e(s)).abs() + e(t).abs())
    if res is not None:
        r = res.double().view(B, Np, Cc)
        if rs is not None:
            bnd = bnd + 2 * U * ((r * e(rs)).abs() + e(rt).abs())
            r = r * e(rs) + e(rt)
        if res_relu:
            r = r.clamp_min(0)
        v = (r + v).clamp_min(0)
        bnd = bnd + U * v.abs()
    return v.view(B * Np, Cc), bnd.view(B * Np, Cc)


def ref_norm_bwd(dy, x, s, t, relu, instance, B, Np, Cc, mut=None, nblk=None):
    e = lambda p: p.double().view(B, 1, Cc)                                      # noqa: E731
    xv, g0 = x.double().view(B, Np, Cc), dy.double().view(B, Np, Cc)
    S, T = e(s), e(t)
    xh = xv * S + T
    e_xh = 2 * U * ((xv * S).abs() + T.abs())
    flip = (xh.abs() <= e_xh) & bool(relu)
    g = torch.where((xh > 0) | (not relu), g0, torch.zeros_like(g0))
    fl = g0.abs() * flip
    if not instance:
        return (S * g).view(-1, Cc), (U * (S * g).abs() + S.abs() * fl).view(-1, Cc)
    gs, gxs = g, g * xh
    if mut == "drop_chunk":
        last = last_chunk_start(Np, nblk)
        gs, gxs = g[:, :last], (g * xh)[:, :last]
    m1, m2 = gs.sum(1, keepdim=True) / Np, gxs.sum(1, keepdim=True) / Np
    e1 = U * m1.abs() + fl.mean(1, keepdim=True)
    e2 = U * m2.abs() + (g.abs() * e_xh).mean(1, keepdim=True) + (fl * (xh.abs() + e_xh)).mean(1, keepdim=True)
    dx = S * ((g - m1) - xh * m2)
    bnd = S.abs() * (fl + e1 + xh.abs() * e2 + e_xh * m2.abs() + 3 * U * (g.abs() + m1.abs() + (xh * m2).abs()))
    return dx.view(-1, Cc), bnd.view(-1, Cc)


def run_norm(lib, stat_name, dev, run):
    B, Np, nblk = STAT_SHAPES[stat_name.split("_c")[0]]
    for Cc in widths_of(stat_name):
        gen = torch.Generator().manual_seed(31 + Cc + Np)
        y = (torch.randn(B * Np, Cc, generator=gen) + torch.randn(1, Cc, generator=gen) * 0.5).to(dev)     # variance ~1, |mean| < ~1.5
        res = torch.randn(B * Np, Cc, generator=gen).to(dev)
        dy = torch.randn(B * Np, Cc, generator=gen).to(dev)
        st = torch.full((4, B, Cc), SENT_F32, device=dev)
        part = torch.zeros(B * nblk * Cc * 2, dtype=torch.float64, device=dev)
        lib.channel_stats(y, B, Np, Cc, st[1], st[2], part, nblk)
        ref = ref_stats(y, B, Np, Cc)
        run.cmp("channel_stats", f"scale C={Cc}", st[1], *ref["scale"])
        run.cmp("channel_stats", f"shift C={Cc}", st[2], *ref["shift"])
        run.sentinel("channel_stats", "neighbouring rows", st[[0, 3]])
        sc, sh = st[1].contiguous(), st[2].contiguous()
        rs, rt = torch.empty(B, Cc, device=dev), torch.empty(B, Cc, device=dev)
        lib.channel_stats(res, B, Np, Cc, rs, rt, part, nblk)
        for name, kw in (("plain", {}), ("res", dict(res=res)), ("rs_rt", dict(res=res, rs=rs, rt=rt)),
                         ("res_relu", dict(res=res, rs=rs, rt=rt, res_relu=True))):
            out = torch.full((B * Np + 2, Cc), SENT_F32, device=dev)
            lib.norm_act(y, sc, sh, out[1:-1], B, Np, Cc, **kw)
            run.cmp("norm_act", f"{name} C={Cc}", out[1:-1], *ref_norm_act(y, sc, sh, B, Np, Cc, **kw))
            run.sentinel("norm_act", "rows around the output", out[[0, -1]])
        fs = (torch.rand(B, Cc, generator=gen) + 0.5).to(dev)
        ft = (torch.rand(B, Cc, generator=gen) - 0.5).to(dev)
        if nblk > Np:                       # pf_norm_bwd takes at most one chunk per pixel (pf_channel_stats takes empty ones)
            from prior_flow_amd._lib import PfError
            try:
                lib.norm_bwd(dy, y, sc, sh, True, True, torch.empty_like(y), B, Np, Cc, nblk=nblk)
            except PfError:
                pass
            else:
                run.fails.append(f"norm_bwd [{run.shape}]: nblk > Np was accepted")
        for relu in (True, False):
            for instance in (True, False):
                s, t = (sc, sh) if instance else (fs, ft)
                dx = torch.full((B * Np + 2, Cc), SENT_F32, device=dev)
                lib.norm_bwd(dy, y, s, t, relu, instance, dx[1:-1], B, Np, Cc, nblk=min(nblk, Np) if instance else None)
                run.cmp("norm_bwd", f"instance={instance} relu={relu} C={Cc}", dx[1:-1],
                        *ref_norm_bwd(dy, y, s, t, relu, instance, B, Np, Cc))
                run.sentinel("norm_bwd", "rows around dx", dx[[0, -1]])


# ------------------------------------------------------------------------------------------------------------------------
# family: bn  (bn_frozen_fwd / bn_frozen_bwd, accumulate on and off)
# ------------------------------------------------------------------------------------------------------------------------
BN_ROWS = OrderedDict(r1=1, r17=17, r200=200, r459=459, rows=ROWS_B * 256)


def ref_bn(x, dy, gamma, beta, mean, var, eps, relu, dg0, db0, accumulate, mut=None, nblk=None):
    D = lambda t: t.double()                                                     # noqa: E731
    x, dy, gamma, beta, mean, var = map(D, (x, dy, gamma, beta, mean, var))
    rows = x.shape[0]
    rstd = 1.0 / torch.sqrt(var + eps)
    s = gamma * rstd
    e_s = 6 * U * s.abs()                                   # var + eps, sqrt (2), 1 / (2), gamma *
    t = beta - mean * s
    e_t = mean.abs() * e_s + U * (mean * s).abs() + U * t.abs()
    yv = x * s + t
    e_y = x.abs() * e_s + e_t + 2 * U * ((x * s).abs() + t.abs())
    out = yv.clamp_min(0) if relu else yv
    flip = (yv.abs() <= e_y) & bool(relu)
    g = torch.where((yv > 0) | (not relu), dy, torch.zeros_like(dy))
    fl = dy.abs() * flip
    dx = s * g
    xhat = (x - mean) * rstd
    gx = g * xhat
    if mut == "drop_chunk":
        last = last_chunk_start(rows, nblk)
        g, gx = g[:last], gx[:last]
    dgam, dbet = gx.sum(0), g.sum(0)
    b_g = 6 * U * gx.abs().sum(0) + (fl * xhat.abs()).sum(0) + U * dgam.abs() + rows * U64 * gx.abs().sum(0)      # xhat: 6 roundings
    b_b = fl.sum(0) + U * dbet.abs() + rows * U64 * g.abs().sum(0)
    if accumulate:
        dgam, dbet = D(dg0) + dgam, D(db0) + dbet
        b_g, b_b = b_g + U * (D(dg0).abs() + dgam.abs()), b_b + U * (D(db0).abs() + dbet.abs())
    b_dx = e_s * dy.abs() + U * dx.abs() + s.abs() * fl
    return dict(out=(out, e_y), dx=(dx, b_dx), dgamma=(dgam, b_g), dbeta=(dbet, b_b))


def run_bn(lib, rows_name, dev, run):
    rows = BN_ROWS[rows_name.split("_c")[0]]
    for Cc in widths_of(rows_name):
        gen = torch.Generator().manual_seed(41 + Cc + rows)
        x = torch.randn(rows, Cc, generator=gen).to(dev)
        dy = torch.randn(rows, Cc, generator=gen).to(dev)
        gamma = (torch.rand(Cc, generator=gen) + 0.5).to(dev)
        beta = (torch.randn(Cc, generator=gen) * 0.3).to(dev)
        mean = (torch.randn(Cc, generator=gen) * 0.2).to(dev)
        var = (torch.rand(Cc, generator=gen) + 0.3).to(dev)
        for relu in (True, False):
            out = torch.full((rows + 2, Cc), SENT_F32, device=dev)
            lib.bn_frozen_fwd(x, gamma, beta, mean, var, 1e-5, relu, out[1:-1])
            for accumulate in (True, False):
                dg0, db0 = rnd(gen, (Cc,), -2, 2, dev), rnd(gen, (Cc,), -2, 2, dev)
                ref = ref_bn(x, dy, gamma, beta, mean, var, EPS_NORM, relu, dg0, db0, accumulate)
                dx = torch.full((rows + 2, Cc), SENT_F32, device=dev)
                dg, db = dg0.clone(), db0.clone()
                lib.bn_frozen_bwd(dy, x, gamma, beta, mean, var, 1e-5, relu, dx[1:-1], dg, db, accumulate)
                tag = f"relu={relu} acc={accumulate} C={Cc}"
                run.cmp("bn_frozen_bwd", "dx " + tag, dx[1:-1], *ref["dx"])
                run.cmp("bn_frozen_bwd", "dgamma " + tag, dg, *ref["dgamma"])
                run.cmp("bn_frozen_bwd", "dbeta " + tag, db, *ref["dbeta"])
                run.sentinel("bn_frozen_bwd", "rows around dx", dx[[0, -1]])
            run.cmp("bn_frozen_fwd", f"out relu={relu} C={Cc}", out[1:-1], *ref["out"])
            run.sentinel("bn_frozen_fwd", "rows around the output", out[[0, -1]])


# ------------------------------------------------------------------------------------------------------------------------
# family: loss_opt  (seq_loss, seq_loss_batch, sum_squares, adamw_step, adamw_step_dev)
# ------------------------------------------------------------------------------------------------------------------------
LOSS_SHAPES = OrderedDict(ragged=(3, 17, 27, 7), even=(2, 16, 32, 3))           # B, h, w, nblk: 459 = 6 * 66 + 63; 512 = 2 * 171 + 170


def ref_seq_loss(pred, gt, valid, w, i_weight, max_flow, nblk, mut=None):
    """partials [B, nblk, 6] and the gradient seed, float64, with bounds.  A pixel whose |gt| is within its rounding of max_flow,
    or whose epe is within its rounding of a 1 / 3 / 5 px threshold, may be counted either way."""
    D = lambda t: t.double()                                                     # noqa: E731
    B, _, h, ww = pred.shape
    N = h * ww
    p, g, va, wt = D(pred).view(B, 2, N), D(gt).view(B, 2, N), D(valid).view(B, N), D(w).view(1, N)
    du, dv = p[:, 0] - g[:, 0], p[:, 1] - g[:, 1]
    mag = torch.sqrt(g[:, 0] ** 2 + g[:, 1] ** 2)
    unsure = (mag - max_flow).abs() <= 4 * U * mag
    ok = (va >= 0.5) & (mag < max_flow)
    m = wt * ok
    iw = float(np.float32(i_weight))
    gs = iw * m
    grad = torch.stack([torch.sign(du) * gs, torch.sign(dv) * gs], 1).view(B, 2, h, ww)
    gb = torch.stack([U * gs + iw * wt * unsure] * 2, 1).view(B, 2, h, ww)
    l1 = m * (du.abs() + dv.abs())
    e = torch.sqrt(du * du + dv * dv)
    cols = [l1, e * ok, ok.double()] + [((e < th) & ok).double() for th in (1.0, 3.0, 5.0)]
    errs = [4 * U * l1 + wt * (du.abs() + dv.abs()) * unsure, 4 * U * e * ok + e * unsure, unsure.double()] + \
           [(((e - th).abs() <= 4 * U * e) | unsure).double() for th in (1.0, 3.0, 5.0)]
    chunk = -(-N // nblk)
    ref = torch.zeros(B, nblk, 6, dtype=torch.float64, device=p.device)
    bnd = torch.zeros_like(ref)
    for k in range(nblk):
        lo, hi = k * chunk, min(N, (k + 1) * chunk)
        if mut == "drop_chunk" and lo == last_chunk_start(N, nblk):
            break
        for j in range(6):
            ref[:, k, j] = cols[j][:, lo:hi].sum(1)
            bnd[:, k, j] = errs[j][:, lo:hi].sum(1) + (hi - lo) * U64 * cols[j][:, lo:hi].abs().sum(1)
    return dict(partials=(ref, bnd), grad=(grad, gb))


def ref_adamw(p, g, m, v, lr, b1, b2, eps, wd, step, gscale):
    """One AdamW step in float64 from the fp32 state (p, g, m, v); the scalars rounded to fp32 as the C entry point does.
    Returns the references, the bounds and the four derived scalars for pf_adamw_step_dev."""
    D = lambda t: t.double()                                                     # noqa: E731
    f32 = lambda a: float(np.float32(a))                                         # noqa: E731
    decay = f32(1.0 - lr * wd)
    sbc2, gs = f32(math.sqrt(1.0 - f32(b2) ** step)), f32(gscale)
    b1, b2, eps = f32(b1), f32(b2), f32(eps)
    step_size = f32(lr / (1.0 - b1 ** step))
    p, g0, m0, v0 = D(p), D(g), D(m), D(v)
    g = g0 * gs
    e_g = U * g.abs()
    mm = m0 + (g - m0) * (1.0 - b1)
    e_m = (1.0 - b1) * e_g + 4 * U * (m0.abs() + (g - m0).abs() * (1.0 - b1))
    vv = v0 * b2 + (g * g) * (1.0 - b2)
    e_v = 2 * g.abs() * e_g * (1.0 - b2) + 5 * U * ((v0 * b2).abs() + g * g * (1.0 - b2))
    sq = torch.sqrt(vv)
    e_sq = torch.minimum(e_v / (2 * sq).clamp_min(1e-300), torch.sqrt(e_v)) + 2 * U * sq
    den = sq / sbc2 + eps
    e_den = e_sq / sbc2 + 3 * U * den
    ratio_ = mm / den
    e_ratio = e_m / den + ratio_.abs() * e_den / den + 2 * U * ratio_.abs()
    pd = p * decay
    pn = pd + ratio_ * (-step_size)
    e_p = U * pd.abs() + step_size * e_ratio + 2 * U * (ratio_ * step_size).abs() + U * pn.abs()
    hyper = torch.tensor([decay, step_size, sbc2, gs], dtype=torch.float32)
    return dict(p=(pn, e_p), m=(mm, e_m), v=(vv, e_v)), hyper


def run_loss_opt(lib, shape, dev, run):
    B, h, w, nblk = LOSS_SHAPES[shape]
    gen = torch.Generator().manual_seed(51 + h)
    gt = rnd(gen, (B, 2, h, w), -40, 40, dev)
    gt[:, :, 0, :3] = 300.0                                  # beyond max_flow
    preds = [(gt + torch.randn(B, 2, h, w, generator=gen).to(dev) * s).contiguous() for s in (0.5, 2.0, 4.0)]
    preds[0][:, :, 1, :5] = gt[:, :, 1, :5]                  # zero difference: zero gradient
    valid = (torch.rand(B, h, w, generator=gen) > 0.2).float().to(dev)
    wt = po.spherical_mask(h, w).contiguous().view(-1).to(dev)
    iws = [0.8 ** 2, 0.8, 1.0]
    parts = torch.full((3, B, nblk, 6), 7.0, dtype=torch.float64, device=dev)
    grads = [torch.full((B, 2, h, w), SENT_F32, device=dev) for _ in preds]
    lib.seq_loss_batch(preds, gt, valid, wt, iws, 400.0, grads, parts)
    for i, (p, iw) in enumerate(zip(preds, iws)):
        ref = ref_seq_loss(p, gt, valid, wt, iw, 400.0, nblk)
        run.cmp("seq_loss_batch", f"partials {i}", parts[i], *ref["partials"])
        run.cmp("seq_loss_batch", f"grad {i}", grads[i], *ref["grad"])
        part = torch.full((B, nblk, 6), 7.0, dtype=torch.float64, device=dev)
        gr = torch.full((B + 2, 2, h, w), SENT_F32, device=dev)
        lib.seq_loss(p, gt, valid, wt, iw, 400.0, gr[1:-1], part)
        run.cmp("seq_loss", f"partials {i}", part, *ref["partials"])
        run.cmp("seq_loss", f"grad {i}", gr[1:-1], *ref["grad"])
        run.sentinel("seq_loss", "images around the gradient", gr[[0, -1]])
    # sum of squares: n not a multiple of 4, ragged last chunk (and chunks past the end when nblk > n)
    for n, nb in ((1031, 7), (5, 8), (B * h * w * 2 + 3, 64)):
        x = torch.randn(n, generator=gen).to(dev)
        part = torch.full((nb + 1,), 7.0, dtype=torch.float64, device=dev)
        lib.sum_squares(x, part[:nb])
        ref, bnd = ref_sum_squares(x, nb)
        run.cmp("sum_squares", f"n={n} nblk={nb}", part[:nb], ref, bnd)
        run.cmp("sum_squares", "partial past the end", part[nb:], torch.full((1,), 7.0, dtype=torch.float64, device=dev), 0.0)
    # AdamW, 3 steps; adamw_step_dev on a copy of the state with the scalars adamw_step derives
    n = 1031 if shape == "ragged" else 4096
    p = torch.randn(n, generator=gen).to(dev)
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    for k in range(3):
        g = (torch.randn(n, generator=gen) * 0.1).to(dev)
        g[::97] = 0.0
        lr, c = 1e-4 * (k + 1) / 3, 0.7 + 0.1 * k
        ref, hyper = ref_adamw(p, g, m, v, lr, 0.9, 0.999, 1e-8, 5e-5, k + 1, c)
        st = torch.full((5, n), SENT_F32, device=dev)
        st[1], st[2], st[3] = p, m, v
        lib.adamw_step_dev(st[1], g, st[2], st[3], 0.9, 0.999, 1e-8, hyper.to(dev))
        lib.adamw_step(p, g, m, v, lr, 0.9, 0.999, 1e-8, 5e-5, k + 1, c)
        for name, a, b in (("p", p, st[1]), ("m", m, st[2]), ("v", v, st[3])):
            run.cmp("adamw_step", f"{name} step {k + 1}", a, *ref[name])
            run.cmp("adamw_step_dev", f"{name} step {k + 1}", b, *ref[name])
        run.sentinel("adamw_step_dev", "rows around the state", st[[0, 4]])


def ref_sum_squares(x, nblk, mut=None):
    n = x.numel()
    chunk = -(-n // nblk)
    ref = torch.zeros(nblk, dtype=torch.float64, device=x.device)
    bnd = torch.zeros_like(ref)
    for k in range(nblk):
        lo, hi = k * chunk, min(n, (k + 1) * chunk)
        if hi > lo:
            ref[k] = (x[lo:hi].double() ** 2).sum()
            bnd[k] = (hi - lo + 1) * U64 * ref[k]
    return ref, bnd


# ------------------------------------------------------------------------------------------------------------------------
# family: warp  (warp_gcorr with both add_grid values, warp_gcorr_bwd)
# ------------------------------------------------------------------------------------------------------------------------
def warp_case(shape, dev, add_grid, seed=5, Cc=256):
    B, H, W = SHAPES[shape]
    R = B * H * W
    gen = torch.Generator().manual_seed(seed + int(add_grid))
    c = dict(shape=shape, B=B, H=H, W=W, R=R, C=Cc, add_grid=add_grid)
    co = edge_coords(f"el/warp/{shape}", B, H, W, gen)
    if add_grid:
        co = (co - po.coords_grid(B, H, W)).contiguous()          # the kernel adds the grid back: one more rounding
    c["coords"] = co.to(dev)
    c["f1"], c["f2"] = rnd(gen, (R, Cc), -1.7, 1.7, dev), rnd(gen, (R, Cc), -1.7, 1.7, dev)
    c["d_flaw"] = rnd(gen, (R, 4), -1, 1, dev)
    c["d_f1_0"], c["d_f2_0"] = rnd(gen, (R, Cc), -1, 1, dev), rnd(gen, (R, Cc), -1, 1, dev)
    return c


def warp_geometry(c):
    """x, y, dx, dy, seam [B, N] of pf_warp_taps."""
    B, H, W = c["B"], c["H"], c["W"]
    N = H * W
    co = c.get("coords64", c["coords"]).double().view(B, 2, N)
    x, y = co[:, 0], co[:, 1]
    ex = ey = torch.zeros_like(x)
    if c["add_grid"]:
        n = torch.arange(N, device=x.device)
        x, y = x + (n % W).double(), y + torch.div(n, W, rounding_mode="floor").double()
        ex, ey = U * x.abs(), U * y.abs()
    xw = torch.remainder(x, W)
    seam = ((W - xw) <= ex) & bool(c["add_grid"])
    if "coord_err" in c:              # the sampled point is itself a computed value (motion_prep): a two-sided error
        ex, ey = ex + c["coord_err"][0], ey + c["coord_err"][1]
        seam = ((W - xw) <= ex) | (xw <= ex)
    return xw, y, ex + U * W + rt_err(xw, W), ey + rt_err(y, H), seam


def ref_warp(c, mut=None):
    """warped f2 [B, N, C] with its bound, and the four group means [R, 4]."""
    B, H, W, Cc = c["B"], c["H"], c["W"], c["C"]
    N = H * W
    x, y, dx, dy, seam = warp_geometry(c)
    taps, (_, _, wx, wy) = taps0(H, W, x, y, mut)
    f2 = c["f2"].double().view(B, N, Cc)
    vals = [torch.gather(f2, 1, idx.unsqueeze(-1).expand(B, N, Cc)) * ok.unsqueeze(-1) for idx, _, ok in taps]
    ws = [w.unsqueeze(-1) for _, w, _ in taps]
    warped = sum(v * w for v, w in zip(vals, ws))
    absw = sum((v * w).abs() for v, w in zip(vals, ws))
    Dx = torch.maximum((vals[1] - vals[0]).abs(), (vals[3] - vals[2]).abs())
    Dy = torch.maximum((vals[2] - vals[0]).abs(), (vals[3] - vals[1]).abs())
    L = 2.0 * f2.abs().amax(1, keepdim=True)                                     # [B, 1, C]
    near = ((torch.minimum(wx, 1.0 - wx) <= dx) | (torch.minimum(wy, 1.0 - wy) <= dy)).unsqueeze(-1)
    Dx, Dy = torch.where(near, L.expand_as(Dx), Dx), torch.where(near, L.expand_as(Dy), Dy)
    bw = dx.unsqueeze(-1) * Dx + dy.unsqueeze(-1) * Dy + M_BILIN * U * absw + seam.unsqueeze(-1) * L
    f1 = c["f1"].double().view(B, N, Cc)
    cg = Cc // 4
    grp = lambda t: t.view(B, N, 4, cg).sum(-1)                                  # noqa: E731
    out = grp(f1 * warped) / cg
    bnd = (grp(f1.abs() * bw) + (cg + 1) * U * grp((f1 * warped).abs())) / cg + U * out.abs()
    return warped, bw, out.view(B * N, 4), bnd.view(B * N, 4)


def scatter_mats(H, W, x, y, dx, dy, seam):
    """Dense [Bm, N_dst, N_src] float64 matrices of a bilinear scatter whose source n has the taps of (x, y)[.., n]: weights,
    coordinate-error budgets (charged to the cells of the taps, and to the 4 x 4 neighbourhood, cyclic in x, for a source
    within its error of an integer coordinate or of the seam -- there the whole weight), contribution counts."""
    Bm, N = x.shape
    taps, (fx, fy, wx, wy) = taps0(H, W, x, y)
    z = lambda: torch.zeros(Bm, N, N, dtype=torch.float64, device=x.device)      # noqa: E731
    S, E, Cn = z(), z(), z()
    bi = torch.arange(Bm, device=x.device).view(Bm, 1).expand(Bm, N)
    src = torch.arange(N, device=x.device).view(1, N).expand(Bm, N)
    dxy = dx + dy
    for idx, w, ok in taps:
        S.index_put_((bi, idx, src), w, accumulate=True)
        E.index_put_((bi, idx, src), dxy * ok, accumulate=True)
        Cn.index_put_((bi, idx, src), (w != 0).double(), accumulate=True)
    near = (torch.minimum(wx, 1.0 - wx) <= dx) | (torch.minimum(wy, 1.0 - wy) <= dy) | seam
    budget = torch.where(seam, torch.ones_like(dxy), dxy) * near
    for oy in (-1, 0, 1, 2):
        yy = fy + oy
        oky = (yy >= 0) & (yy <= H - 1)
        for ox in (-1, 0, 1, 2):
            cell = (yy.clamp(0, H - 1) * W + torch.remainder(fx + ox, W)).long()
            E.index_put_((bi, cell, src), budget * oky, accumulate=True)
    return S, E, Cn


def ref_warp_bwd(c, launches=1):
    B, H, W, Cc = c["B"], c["H"], c["W"], c["C"]
    N = H * W
    cg = Cc // 4
    warped, bw, _, _ = ref_warp(c)
    gs = (c["d_flaw"].double() / cg).view(B, N, 4, 1).expand(B, N, 4, cg).reshape(B, N, Cc)
    e_gs = U * gs.abs()
    d1_0, d2_0 = c["d_f1_0"].double().view(B, N, Cc), c["d_f2_0"].double().view(B, N, Cc)
    add1 = gs * warped
    d1 = d1_0 + launches * add1
    b1 = launches * (gs.abs() * bw + e_gs * warped.abs() + U * add1.abs()) + (launches + 1) * U * (d1_0.abs() + launches * add1.abs())
    x, y, dx, dy, seam = warp_geometry(c)
    S, E, Cn = scatter_mats(H, W, x, y, dx, dy, seam)
    V = gs * c["f1"].double().view(B, N, Cc)
    add2, A = torch.matmul(S, V), torch.matmul(S, V.abs())
    n = Cn.sum(2).unsqueeze(-1)
    d2 = d2_0 + launches * add2
    b2 = launches * (torch.matmul(E, V.abs()) + 6 * U * A) + (launches * n + 1) * U * (d2_0.abs() + launches * A)
    return dict(d_f1=(d1.view(-1, Cc), b1.view(-1, Cc)), d_f2=(d2.view(-1, Cc), b2.view(-1, Cc)))


def _warp(lib, shape, dev, run):
    # `rows_c64` is the 66 560-row case with 64 instead of 256 channels (four per group)
    base, Cc = (shape.split("_c")[0], int(shape.split("_c")[1])) if "_c" in shape else (shape, 256)
    for add_grid, (ld, off) in ((False, (9, 1)), (True, (8, 4))):
        c = warp_case(base, dev, add_grid, Cc=Cc)
        name = "warp_gcorr+grid" if add_grid else "warp_gcorr"
        _, _, ref, bnd = ref_warp(c)
        dst = torch.full((c["R"], ld), SENT_F32, device=dev)
        lib.warp_gcorr(c["f1"], c["f2"], c["coords"], add_grid, dst, off)
        run.cmp(name, "group means", dst[:, off:off + 4], ref, bnd)
        run.sentinel(name, "other columns", outside(dst, off, 4))
        d_flaw, _ = padded(c["d_flaw"], ld, off)
        d1, d2 = c["d_f1_0"].clone(), c["d_f2_0"].clone()
        lib.warp_gcorr_bwd(c["f1"], c["f2"], c["coords"], add_grid, d_flaw, off, d1, d2)
        refb = ref_warp_bwd(c)
        run.cmp("warp_gcorr_bwd", f"d_f1 add_grid={add_grid}", d1, *refb["d_f1"])
        run.cmp("warp_gcorr_bwd", f"d_f2 add_grid={add_grid}", d2, *refb["d_f2"])
        run.sentinel("warp_gcorr_bwd", "d_flaw padding", outside(d_flaw, off, 4))


# ------------------------------------------------------------------------------------------------------------------------
# family: upsample  (upsample_flow, upsample_flow_bwd) and flow_head_out
# ------------------------------------------------------------------------------------------------------------------------
EPS_TRANS = 2.0 ** -20               # device expf / division on values <= 1 (tests/conv_launches.py)


def _softmax9(mask, B, H, W):
    """w [B, 9, 8, 8, H, W] = softmax_k(mask[.., 64k + 8i + j]) and its bound: expf of l - max (EPS_TRANS absolute, the
    subtraction 2 U |l - max| relative), nine additions, the division."""
    lg = mask.double().view(B, H, W, 9, 8, 8).permute(0, 3, 4, 5, 1, 2)
    d = lg - lg.amax(1, keepdim=True)
    e = torch.exp(d)
    e_e = EPS_TRANS + 2 * U * d.abs() * e
    den = e.sum(1, keepdim=True)
    e_den = e_e.sum(1, keepdim=True) + 9 * U * den
    w = e / den
    return w, (e_e + w * e_den) / den + 2 * U * w + EPS_TRANS * w


def _nb_flow(coords1, B, H, W):
    """8 * flow at the nine 3 x 3 neighbours, zero outside: [B, 2, 9, H, W], its rounding bound, and the in-range mask."""
    fl = 8.0 * (coords1.double() - po.coords_grid(B, H, W).to(coords1.device).double())
    pad = torch.nn.functional.pad(fl, (1, 1, 1, 1))
    nb = torch.stack([pad[:, :, k // 3:k // 3 + H, k % 3:k % 3 + W] for k in range(9)], 2)
    return nb, U * nb.abs()


def ref_upsample(coords1, mask, B, H, W, mut=None):
    w, e_w = _softmax9(mask, B, H, W)
    nb, e_nb = _nb_flow(coords1, B, H, W)
    nbx = nb.view(B, 2, 9, 1, 1, H, W)
    out = (w.unsqueeze(1) * nbx).sum(2)                                         # [B, 2, 8, 8, H, W]
    bnd = (e_w.unsqueeze(1) * nbx.abs() + w.unsqueeze(1) * e_nb.view(B, 2, 9, 1, 1, H, W)).sum(2) + 11 * U * (w.unsqueeze(1) * nbx.abs()).sum(2)
    fine = lambda t: t.permute(0, 1, 4, 2, 5, 3).reshape(B, 2, 8 * H, 8 * W)     # noqa: E731
    return fine(out), fine(bnd)


def ref_upsample_bwd(coords1, mask, g, d_flow0, B, H, W, launches=1):
    w, e_w = _softmax9(mask, B, H, W)
    nb, e_nb = _nb_flow(coords1, B, H, W)
    gg = g.double().view(B, 2, H, 8, W, 8).permute(0, 1, 3, 5, 2, 4)             # [B, 2, 8, 8, H, W]
    gu, gv = gg[:, 0:1], gg[:, 1:2]                                              # [B, 1, 8, 8, H, W]
    fu, fv = nb[:, 0].view(B, 9, 1, 1, H, W), nb[:, 1].view(B, 9, 1, 1, H, W)
    eu, ev = e_nb[:, 0].view(B, 9, 1, 1, H, W), e_nb[:, 1].view(B, 9, 1, 1, H, W)
    s = gu * fu + gv * fv                                                        # [B, 9, 8, 8, H, W]
    e_s = gu.abs() * eu + gv.abs() * ev + 3 * U * ((gu * fu).abs() + (gv * fv).abs())
    dot = (w * s).sum(1, keepdim=True)
    e_dot = (e_w * s.abs() + w * e_s).sum(1, keepdim=True) + 11 * U * (w * s).abs().sum(1, keepdim=True)
    dm = w * (s - dot)
    b_dm = e_w * (s - dot).abs() + w * (e_s + e_dot) + 2 * U * (w * (s.abs() + dot.abs()))
    rows = lambda t: t.permute(0, 4, 5, 1, 2, 3).reshape(B * H * W, 576)         # noqa: E731
    # d_flow[neighbour k of (y, x)] += 8 w_k g over the 64 sub-pixels: sum them, then shift the 9 planes onto their neighbours
    acc = torch.zeros(B, 2, H + 2, W + 2, dtype=torch.float64, device=g.device)
    A, Eb, n = torch.zeros_like(acc), torch.zeros_like(acc), torch.zeros_like(acc)
    for k in range(9):
        sl = (slice(None), slice(None), slice(k // 3, k // 3 + H), slice(k % 3, k % 3 + W))
        cu = 8.0 * w[:, k:k + 1] * gg                                            # [B, 2, 8, 8, H, W]
        acc[sl] += cu.sum((2, 3))
        A[sl] += cu.abs().sum((2, 3))
        Eb[sl] += (8.0 * e_w[:, k:k + 1] * gg.abs()).sum((2, 3))
        n[sl] += 64.0
    core = (slice(None), slice(None), slice(1, H + 1), slice(1, W + 1))
    d0 = d_flow0.double()
    df = d0 + launches * acc[core]
    b_df = launches * (Eb[core] + 3 * U * A[core]) + (launches * n[core] + 1) * U * (d0.abs() + launches * A[core])
    return dict(d_mask=(rows(dm), rows(b_dm)), d_flow=(df, b_df))


def ref_flow_head(x, w, bias, coords1, B, H, W, Cc):
    F = torch.nn.functional
    xn = x.double().view(B, H, W, -1)[..., :Cc].permute(0, 3, 1, 2)
    wn = w.double().view(2, 3, 3, Cc).permute(0, 3, 1, 2)
    acc = F.conv2d(xn, wn, bias.double(), padding=1)
    mag = F.conv2d(xn.abs(), wn.abs(), bias.double().abs(), padding=1)
    b_acc = (9 * Cc + 2) * U * mag
    c1 = coords1.double() + acc
    return dict(delta=(acc, b_acc), coords1=(c1, b_acc + U * c1.abs()))


def _upsample(lib, shape, dev, run):
    B, H, W = SHAPES[shape]
    R = B * H * W
    gen = torch.Generator().manual_seed(61)
    coords1 = (po.coords_grid(B, H, W) + (torch.rand(B, 2, H, W, generator=gen) * 12 - 6)).contiguous().to(dev)
    mask, _ = padded(rnd(gen, (R, 576), -2, 2, dev), 577)
    up = torch.full((B + 2, 2, 8 * H, 8 * W), SENT_F32, device=dev)
    lib.upsample_flow(coords1, mask, up[1:-1])
    run.cmp("upsample_flow", "out", up[1:-1], *ref_upsample(coords1, mask[:, :576], B, H, W))
    run.sentinel("upsample_flow", "images around the output", up[[0, -1]])
    g = rnd(gen, (B, 2, 8 * H, 8 * W), -1, 1, dev)
    d_flow0 = rnd(gen, (B, 2, H, W), -1, 1, dev)
    d_flow = d_flow0.clone()
    d_mask = torch.full((R, 580), SENT_F32, device=dev)
    lib.upsample_flow_bwd(coords1, mask, g, d_mask, d_flow)
    ref = ref_upsample_bwd(coords1, mask[:, :576], g, d_flow0, B, H, W)
    run.cmp("upsample_flow_bwd", "d_mask", d_mask[:, :576], *ref["d_mask"])
    run.cmp("upsample_flow_bwd", "d_flow", d_flow, *ref["d_flow"])
    run.sentinel("upsample_flow_bwd", "d_mask padding", d_mask[:, 576:])
    run.sentinel("upsample_flow", "mask padding", mask[:, 576:])


def _flow_head(lib, shape, dev, run, Cc=256):
    B, H, W = SHAPES[shape]
    R = B * H * W
    gen = torch.Generator().manual_seed(71)
    w = rnd(gen, (2, 9, Cc), -0.05, 0.05, dev)
    bias = rnd(gen, (2,), -0.1, 0.1, dev)
    co = edge_coords(f"el/fho/{shape}", B, H, W, gen).to(dev)
    for ld, ldd in ((Cc, 4), (Cc + 1, 3)):
        x, _ = padded(rnd(gen, (R, Cc), -1, 1, dev), ld)
        ref = ref_flow_head(x, w, bias, co, B, H, W, Cc)
        rows = lambda t: t.permute(0, 2, 3, 1).reshape(R, 2)                     # noqa: E731
        c1 = co.clone()
        delta = torch.full((R, ldd), SENT_F32, device=dev)
        lib.flow_head_out(x, Cc, w, bias, c1, delta)
        run.cmp("flow_head_out", f"delta ld={ld}", delta[:, :2], rows(ref["delta"][0]), rows(ref["delta"][1]))
        run.cmp("flow_head_out", f"coords1 ld={ld}", c1, *ref["coords1"])
        run.sentinel("flow_head_out", "delta padding", delta[:, 2:])
        c2 = co.clone()
        lib.flow_head_out(x, Cc, w, bias, c2, None)
        run.cmp("flow_head_out", "without the delta buffer", c2, c1.double(), 0.0)


# ------------------------------------------------------------------------------------------------------------------------
# family: rotate  (flo_rotate, motion_prep)
#
# pf_flo_rotate is piecewise smooth: besides the floor flips of its two cyclic gathers it jumps by W where a grid value sits
# half a map away from its anchor (pf_unwrap_m), where the camera-frame flow sits on the +-W/2 clip, and through them in the
# outer mix.  Each of these is detected on the float64 values with the error the fp32 value can have at that point, and the
# jump (W times the weight it enters with) is added to the bound there; everything else is first order as for the gathers:
#   end point   ex = pymod((px + u) + 0.5, W) - 0.5: four roundings of magnitude <= max(|px + u| + 0.5, W), and pf_wraptaps'
#               own pymod (U W); ey = clamp(py + v): U |py + v|;
#   e0, e1      the cyclic bilinear mix of the (unwrapped) grid values: e_x Dx + e_y Dy with the cell's differences (W, the
#               largest circular difference, within the error of an integer), 10 U sum w |value|, 5 U W for pf_unwrap_m;
#   f0          e0 - g0[p], clipped to +-W/2: U (|s| + |s + W/2| + 2 W); within that of the clip: + W;
#   outer mix   sum_j w_j e(F_j) + 10 U sum w_j |F_j|, and U W on the x fraction where g_c2w's x is negative (pymod adds W).
# ------------------------------------------------------------------------------------------------------------------------
def wraptaps64(gx, gy, H, W):
    gxw = torch.remainder(gx, W)
    fx, fy = torch.floor(gxw), torch.floor(gy)
    xw, yw = gxw - fx, gy - fy
    x0 = torch.remainder(fx, W).long()
    x1 = (x0 + 1) % W
    y0, y1 = fy.clamp(0, H - 1).long(), (fy + 1).clamp(0, H - 1).long()
    idx = (y0 * W + x0, y1 * W + x0, y0 * W + x1, y1 * W + x1)                   # a, b, c, d
    w = ((1 - xw) * (1 - yw), (1 - xw) * yw, xw * (1 - yw), xw * yw)
    return idx, w, xw, yw


def ref_flo_rotate(flow, g_w2c, g_c2w, mut=None):
    """flow [B, 2, H, W] fp32 -> (out [B, 2, H, W] float64, bound)."""
    B, _, H, W = flow.shape
    N = H * W
    dev = flow.device
    n = torch.arange(N, device=dev)
    px, py = (n % W).double().view(1, N), torch.div(n, W, rounding_mode="floor").double().view(1, N)
    u, v = flow.double().view(B, 2, N)[:, 0], flow.double().view(B, 2, N)[:, 1]
    g0, g1 = g_w2c.double().view(2, N)[0], g_w2c.double().view(2, N)[1]
    exr = px + u + 0.5
    ex = torch.remainder(exr, W) - 0.5
    e_ex = U * ((px + u).abs() + exr.abs() + 2 * W + ex.abs() + 0.5)
    eyr = py + v
    ey = eyr.clamp(-0.5, H - 0.5)
    e_ey = U * eyr.abs()
    idx, w, xw, yw = wraptaps64(ex, ey, H, W)
    near = (torch.minimum(xw, 1 - xw) <= e_ex) | (torch.minimum(yw, 1 - yw) <= e_ey)
    a0 = g0[idx[0]]
    vals, jump = [a0], torch.zeros_like(a0)
    for j in (1, 2, 3):
        t = torch.remainder(g0[idx[j]] - a0 + W / 2.0, W)
        close = torch.minimum(t, W - t) <= 4 * U * (g0[idx[j]].abs() + a0.abs() + W)
        vals.append(a0 + t - W / 2.0)
        jump = jump + W * w[j] * close
    e0 = sum(wj * vj for wj, vj in zip(w, vals))
    Dx = torch.maximum((vals[2] - vals[0]).abs(), (vals[3] - vals[1]).abs())
    Dy = torch.maximum((vals[1] - vals[0]).abs(), (vals[3] - vals[2]).abs())
    Wt = torch.full_like(Dx, float(W))
    Dx, Dy = torch.where(near, Wt, Dx), torch.where(near, Wt, Dy)
    e_e0 = e_ex * Dx + e_ey * Dy + 10 * U * sum(wj * vj.abs() for wj, vj in zip(w, vals)) + 5 * U * W + jump
    s0 = e0 - g0.view(1, N)
    t = torch.remainder(s0 + W / 2.0, W)
    f0 = t - W / 2.0
    e_f0 = e_e0 + U * (s0.abs() + (s0 + W / 2.0).abs() + 2 * W)
    e_f0 = e_f0 + W * (torch.minimum(t, W - t) <= e_f0)
    v1 = [g1[i] for i in idx]
    e1 = sum(wj * vj for wj, vj in zip(w, v1))
    Dx1 = torch.maximum((v1[2] - v1[0]).abs(), (v1[3] - v1[1]).abs())
    Dy1 = torch.maximum((v1[1] - v1[0]).abs(), (v1[3] - v1[2]).abs())
    L1 = torch.full_like(Dx1, 2.0 * float(g1.abs().max()))
    Dx1, Dy1 = torch.where(near, L1, Dx1), torch.where(near, L1, Dy1)
    f1 = e1 - g1.view(1, N)
    e_f1 = e_ex * Dx1 + e_ey * Dy1 + 10 * U * sum(wj * vj.abs() for wj, vj in zip(w, v1)) + U * f1.abs()
    # outer mix over the camera-frame flow at the four corners of g_c2w (no unwrapping here)
    gcx, gcy = g_c2w.double().view(2, N)[0], g_c2w.double().view(2, N)[1]
    oi, ow, oxw, oyw = wraptaps64(gcx, gcy, H, W)
    if mut == "drop_tap":
        ow = (ow[0], ow[1], ow[2], torch.zeros_like(ow[3]))
    dxo = (U * W * ((gcx < 0) & (gcx > -W))).view(1, N)
    near_o = (torch.minimum(oxw, 1 - oxw).view(1, N) <= dxo) & (dxo > 0)
    outs = []
    for F, eF in ((f0, e_f0), (f1, e_f1)):
        c = [F[:, i] for i in oi]
        o = sum(wj * cj for wj, cj in zip(ow, c))
        Dxo = torch.maximum((c[2] - c[0]).abs(), (c[3] - c[1]).abs())
        Dxo = torch.where(near_o.expand_as(Dxo), 2.0 * F.abs().amax(1, keepdim=True).expand_as(Dxo), Dxo)
        b = sum(wj * eF[:, i] for wj, i in zip(ow, oi)) + 10 * U * sum(wj * cj.abs() for wj, cj in zip(ow, c)) + dxo * Dxo
        outs.append((o, b))
    out = torch.stack([outs[0][0], outs[1][0]], 1).view(B, 2, H, W)
    bnd = torch.stack([outs[0][1], outs[1][1]], 1).view(B, 2, H, W)
    return out, bnd


def rotate_grids(H, W, kind, gen, dev):
    if kind == "real":
        return (po.sample_grid(H, W, po.rotation_x(-math.pi / 2)).contiguous().to(dev),
                po.sample_grid(H, W, po.rotation_x(math.pi / 2)).contiguous().to(dev))
    return grids(H, W, "random", gen, 0).to(dev), grids(H, W, "random", gen, 0).to(dev)


def edge_flows(tag, B, H, W, gen):
    """gc.flows (zero row, +-W/2, clamps at the top and the bottom) on the first images, larger random flows with exact integers
    and multi-wrap x on the others."""
    f = gc.flows(tag, min(B, 2), H, W)
    f = f.repeat((B + f.shape[0] - 1) // f.shape[0], 1, 1, 1)[:B].clone()
    r = (torch.rand(B, 2, H, W, generator=gen) - 0.5) * 24.0
    r[:, :, ::3, ::5] = torch.round(r[:, :, ::3, ::5])
    r[:, 0, 1::4] += 2.5 * W
    r[:, 0, 2::4] -= 1.75 * W
    f[:, :, 6:] = r[:, :, 6:]
    return f.contiguous()


def rows2(t):
    B, _, H, W = t.shape
    return t.permute(0, 2, 3, 1).reshape(B * H * W, 2)


def _rotate(lib, shape, dev, run):
    B, H, W = SHAPES[shape]
    N, R = H * W, B * H * W
    gen = torch.Generator().manual_seed(81)
    for kind in (("real", "random") if shape != "rows" else ("real",)):
        g_w2c, g_c2w = rotate_grids(H, W, kind, gen, dev)
        flow = edge_flows(f"el/rot/{shape}", B, H, W, gen).to(dev)
        ref, bnd = ref_flo_rotate(flow, g_w2c, g_c2w)
        out = torch.full((B + 2, 2, H, W), SENT_F32, device=dev)
        d0 = torch.full((R, 5), SENT_F32, device=dev)
        d1 = torch.full((R, 4), SENT_F32, device=dev)
        lib.flo_rotate(flow, g_w2c, g_c2w, out[1:-1], d0, 1, d1, 2)
        run.cmp("flo_rotate", f"planar, {kind} grids", out[1:-1], ref, bnd)
        run.cmp("flo_rotate", "dst0 is the planar output", d0[:, 1:3], rows2(out[1:-1]).double(), 0.0)
        run.cmp("flo_rotate", "dst1 is the planar output", d1[:, 2:4], rows2(out[1:-1]).double(), 0.0)
        run.sentinel("flo_rotate", "other columns", torch.cat([outside(d0, 1, 2), outside(d1, 2, 2)], 1))
        run.sentinel("flo_rotate", "images around the output", out[[0, -1]])
        # motion_prep: the same rotation of flow_B = coords1_B - coords0 formed in fp32, both flows, both warped correlations
        c0 = po.coords_grid(B, H, W).to(dev)
        c1a = edge_coords(f"el/mp/{shape}", B, H, W, gen).to(dev)
        c1b = (c0 + flow).contiguous()
        fb32, fa32 = c1b - c0, c1a - c0                                 # one fp32 subtraction each: exact against torch
        rba, bba = ref_flo_rotate(fb32, g_w2c, g_c2w)
        wc = warp_case(shape, dev, False, seed=83)
        flow4 = torch.full((R, 4), SENT_F32, device=dev)
        flow2 = torch.full((R, 2), SENT_F32, device=dev)
        conf = torch.full((R, 9), SENT_F32, device=dev)
        xa = torch.full((R, 7), SENT_F32, device=dev)
        xb = torch.full((R, 5), SENT_F32, device=dev)
        lib.motion_prep(c1a, c1b, g_w2c, g_c2w, wc["f1"], wc["f2"], flow4, flow2, conf, xa, 2, xb, 1)
        run.cmp("motion_prep", "flow_A", flow4[:, :2], rows2(fa32).double(), 0.0)
        run.cmp("motion_prep", "flow_B", flow2, rows2(fb32).double(), 0.0)
        run.cmp("motion_prep", f"flow_B_A, {kind} grids", flow4[:, 2:], rows2(rba), rows2(bba))
        run.cmp("motion_prep", "x_a tail", xa[:, 2:6], flow4.double(), 0.0)
        run.cmp("motion_prep", "x_b tail", xb[:, 1:3], flow2.double(), 0.0)
        run.sentinel("motion_prep", "other columns", torch.cat([outside(xa, 2, 4), outside(xb, 1, 2), conf[:, 8:]], 1))
        wc["coords"] = c1a
        _, _, ra, ba = ref_warp(wc)
        run.cmp("motion_prep", "flaw_A", conf[:, :4], ra, ba)
        # flaw_B_A samples at coords0 + flow_B_A: the rotation's bound enters the warp as a coordinate error
        wc["coords"], wc["add_grid"], wc["coord_err"] = rba.float().contiguous(), True, (bba.view(B, 2, N)[:, 0], bba.view(B, 2, N)[:, 1])
        wc["coords64"] = rba
        _, _, rb, bb = ref_warp(wc)
        run.cmp("motion_prep", "flaw_B_A", conf[:, 4:8], rb, bb)


# ------------------------------------------------------------------------------------------------------------------------
# the case table
# ------------------------------------------------------------------------------------------------------------------------
def _lookup(lib, shape, dev, run):
    for kind in (("real", "random") if shape != "rows" else ("random",)):
        run_lookup(lib, lookup_case(shape, dev, kind), run)


def _combine(lib, shape, dev, run):
    for kind in (("real", "random") if shape != "rows" else ("real",)):
        run_combine(lib, combine_case(shape, dev, kind), run)


def _lookup_bwd(lib, shape, dev, run):
    for kind, ld in ((("real", 336), ("random", 325)) if shape != "rows" else (("random", 325),)):
        run_lookup_bwd(lib, lookup_bwd_case(shape, dev, kind), run, ld)


FAMILIES = OrderedDict(
    lookup=(_lookup, tuple(SHAPES), ("dccl_lookup", "dccl_lookup_il")),
    combine=(_combine, tuple(SHAPES), ("dccl_combine", "dccl_combine_bwd")),
    lookup_bwd=(_lookup_bwd, tuple(SHAPES), ("dccl_lookup_bwd",)),
    small=(run_small, tuple(SHAPES), ("pyramid_bwd", "coords_add", "coords_add_to")),
    warp=(_warp, tuple(SHAPES), ("warp_gcorr", "warp_gcorr+grid", "warp_gcorr_bwd")),
    upsample=(_upsample, tuple(SHAPES), ("upsample_flow", "upsample_flow_bwd")),
    flow_head=(_flow_head, tuple(SHAPES), ("flow_head_out",)),
    rotate=(_rotate, tuple(SHAPES), ("flo_rotate", "motion_prep")),
    gru=(run_gru, tuple(ROW_COUNTS), ("gru_q_bwd", "gru_zr_bwd", "gru_dx_finish")),
    norm=(run_norm, tuple(STAT_SHAPES), ("channel_stats", "norm_act", "norm_bwd")),
    bn=(run_bn, tuple(BN_ROWS), ("bn_frozen_fwd", "bn_frozen_bwd")),
    loss_opt=(run_loss_opt, tuple(LOSS_SHAPES), ("seq_loss", "seq_loss_batch", "sum_squares", "adamw_step", "adamw_step_dev")),
)
CASES = [(fam, shape) for fam, (_, shapes, _) in FAMILIES.items() for shape in shapes]

# Cases the host emulation runs as a sibling under a name of its own, so that a table row says what ran: the full-width warp
# over 66 560 rows spends its time in the float64 reference (three dense 260 x 256 x 256 scatter matrices per launch), far beyond
# the other cases on a CPU.  The GPU runs CASES as they are.
CPU_SIBLINGS = {("warp", "rows"): "rows_c64"}


def cases(device_type):
    return [(f, CPU_SIBLINGS.get((f, s), s) if device_type == "cpu" else s) for f, s in CASES]


def run_case(lib, family, shape, dev, table):
    """Runs one (family, shape) case; returns the list of failures (empty = pass).  A kernel of the family that left no row in
    the table at this shape is a failure of the case."""
    run = Run(table, shape)
    FAMILIES[family][0](lib, shape, dev, run)
    run.fails += [f"{k} [{shape}]: not in the table" for k in FAMILIES[family][2] if (k, shape) not in table.rows]
    return run.fails
