"""Launch-level checks of the matrix-core kernels that do not go through pf_conv2d -- the correlation build (pf_corr_pyramid,
pf_corr_pyramid_bf16x3 with pf_split_bf16 / pf_split_f16 and pf_feature_pyramid beside it), the encoders' stem (pf_enc_stem), the
direct and small convolutions (pf_conv2d_direct, pf_conv2d_direct_group[_f16], pf_conv2d_small on each kernel their dispatch
selects), the confidence stem (pf_conf_stem[_f16]) and pf_dccl_combine_conv1x1[_f16] -- against float64 (not a conftest, nothing
here is collected).  The same cases run on the GPU against the HIP library (tests/test_hip_mfma_launches.py) and on the CPU
(tests/test_mfma_launch_reference.py): the entry points the host emulation has (the splits, the feature pyramid, the direct
convolutions, the confidence stem) run on it, the device-only kernels as torch emulations of their arithmetic.

Table, Run, ratio and the sentinels are tests/elem_launches.py's; the two bounds and their constants are tests/conv_launches.py's
(C_ELEM, K_AGG, U_PROD, EPS_EPI, _u_elem, _u_agg), unchanged.  For one output element v = sum_k x_k w_k with
A = sum_k |x_k w_k| and R = sqrt(sum_k (x_k w_k)^2),
    |err| <= C_ELEM * _u_elem(prec, K) * A       (worst case per element)
    |err| <= K_AGG  * _u_agg(prec, K)  * R       (random walk of the per-product errors)
must both hold, so one number per element is compared: |err| / min(the two bounds).  Every further term is a count of fp32
roundings (U = 2^-24 of the magnitude entering the rounding) written next to the reference that uses it:

  corr, level 0      K = C, x = f1[n1], w = f2[n2], everything divided by sqrt(C) in float64.  sqrt(C) a power of two: the scaling
                     is an exact multiplication.  Otherwise the kernel divides by sqrtf(C): one rounding of the divisor and one
                     of the quotient, 2 U (|v| + bound).
  corr, level i + 1  ((c00 + c01) + c10) + c11 times 0.25 (exact): the mean of the four children's bounds plus three additions,
                     each of a partial sum of at most sum |child|, i.e. 3 U sum (|child| + bound) / 4.  Floor semantics: an odd
                     level drops its last row / column.
  feature pyramid    the same pooling statement over channel-last rows; level 0 is the input (bound 0).
  splits             bit for bit, bound 0.
  enc stem           K = 147, bf16x3, plus the bias in A and R and conv_launches' epilogue term EPS_EPI |v|; ReLU is 1-Lipschitz.
                     A twin that is the only output adds its representation error 2^-16 (|v| + bound).  The fused statistics are
                     compared with float64 sums of the kernel's own stored rows per tile: n U64 sum |term| for the n = 256 fp64
                     additions of a tile (elem_launches' channel_stats term); squares of fp32 values are exact in fp64.
  direct / small     K = KH KW Cin with the bias in A and R and EPS_EPI |v|; fp32 for pf_stem7x7c2_valu, pf_small_conv_mfma and
                     pf_direct_conv_elem, bf16x3 (K = 98) for pf_flow_stem_kernel.  A twin or f16 map beside fp32 rows is their
                     split / fp16 rounding bit for bit; alone it adds 2^-16 (|v| + bound) resp. 2^-11 (|v| + bound) + 2^-25.
  conf stem          two chained fp32 3x3 layers (K = 72, 288): the first layer's bound enters the second as sum |w2| bound1 (a
                     float64 convolution of the bound with |w2|); ReLU is 1-Lipschitz, no element is excluded.
  combine + conv1x1  the combined row and its bound are elem_launches.ref_combine's; the 1x1 convolution (K = 324, bf16x3) takes
                     that bound as the input perturbation sum |w| bound.
"""
import math
import os
from collections import OrderedDict

import numpy as np
import torch

import conv_launches as cl
import elem_launches as el
from elem_launches import Run, Table, ratio, U, U64, SENT_F32          # noqa: F401  (re-exported for the two test modules)

SENT_BF16 = cl.SENT_BF16
F32, BF16X3 = 0, 1
PREC = {F32: "fp32", BF16X3: "bf16x3"}


def two_bounds(prec, K, A, R):
    """min of conv_launches' per-element and aggregate bounds."""
    return torch.minimum(cl.C_ELEM * cl._u_elem(prec, K) * A, cl.K_AGG * cl._u_agg(prec, K) * R)


def split_ref(x):
    """hi = bf16(x), lo = bf16(x - hi), as [rows, C/32, 2, 32] (the layout of pf_split_bf16 and of every split twin)."""
    return cl._twin_from(x)


def twin_hi_lo(t):
    """[rows, n, 2, 32] bf16 -> fp32 hi [rows, 32 n], lo [rows, 32 n]."""
    return t[:, :, 0, :].reshape(t.shape[0], -1).float(), t[:, :, 1, :].reshape(t.shape[0], -1).float()


def guarded(rows, width, dev, dtype=torch.float32):
    """[rows, width] filled with NaN inside one allocation with two NaN guard rows (rounded up to 16 bytes) on either side:
    (view, front guard, back guard).  An element a launch does not write stays NaN (ratio inf); a guard it writes shows."""
    g = (2 * width + 3) // 4 * 4
    flat = torch.full((2 * g + rows * width,), float("nan"), dtype=dtype, device=dev)
    return flat[g:g + rows * width].view(rows, width), flat[:g], flat[g + rows * width:]


def pool_floor(t, H, W):
    """[..., H * W] -> the four children [..., (H//2) * (W//2)] of every 2x2 window, floor semantics."""
    v = t.reshape(*t.shape[:-1], H, W)[..., :H // 2 * 2, :W // 2 * 2]
    kids = [v[..., dy::2, dx::2].reshape(*t.shape[:-1], -1) for dy in (0, 1) for dx in (0, 1)]
    return kids


def pool_ref(ref, bnd, H, W):
    """One pooled level in float64 and its bound (module docstring: corr, level i + 1)."""
    kr, kb = pool_floor(ref, H, W), pool_floor(bnd, H, W)
    out = sum(kr) / 4.0
    b = sum(kb) / 4.0 + 3 * U * sum(r.abs() + b_ for r, b_ in zip(kr, kb)) / 4.0
    return out, b


def pool_f32(t, H, W, mut=None):
    """The kernels' pooling in fp32: ((c00 + c01) + c10) + c11, times 0.25.
    mut 'pool_offset': windows taken from pairs offset by one column; 'pool_last': an odd level takes its last row / column into
    the last window instead of dropping it."""
    v = t.reshape(*t.shape[:-1], H, W)
    if mut == "pool_offset":
        v = torch.roll(v, -1, -1)
    if mut == "pool_last":
        if H % 2:
            v = torch.cat([v[..., :H - 3, :], v[..., H - 2:, :], v[..., H - 1:, :]], -2)
        if W % 2:
            v = torch.cat([v[..., :W - 3], v[..., W - 2:], v[..., W - 1:]], -1)
    c = pool_floor(v.reshape(*t.shape[:-1], H * W), H, W)
    return (((c[0] + c[1]) + c[2]) + c[3]) * 0.25


# ------------------------------------------------------------------------------------------------------------------------
# family: corr  (pf_corr_pyramid, pf_split_bf16 + pf_corr_pyramid_bf16x3)
# ------------------------------------------------------------------------------------------------------------------------
def scale_is_exact(C):
    """csrc/pf_corr_mfma.hip:960-964: inv_scale = sqrtf(C); scale_mul != 0 iff inv_scale is a power of two whose square is C."""
    s = float(np.sqrt(np.float32(C), dtype=np.float32))
    m, _ = math.frexp(s)
    return m == 0.5 and s * s == float(C)


def corr_select(B, H8, W8, C, split, rs_on=True):
    """The path corr_launch takes (csrc/pf_corr_mfma.hip), host logic only: (path, RB, chunks, precision, scale branch).
      :951-953  C % 32 == 0, level 3 at least 2 x 2, else no launch (None)
      :967      fused = W8 % 32 == 0 and H8 % 8 == 0 and N % 128 == 0
      :975-977  role-split: fused, split operands, C == 256, W8 % 64 == 0, PRIORFLOW_CORR_RS not '0';
                chunks = 2 if W8 % 128 == 0 else 1, RB = 16 if H8 % 16 == 0 else 8
      :1010-12  otherwise the fused tile kernel, fp32 or split
      :1015-34  not fused: the generic kernel and three pf_pool_kernel passes"""
    if C <= 0 or C % 32 or (H8 >> 3) < 2 or (W8 >> 3) < 2 or B <= 0:
        return None
    prec = PREC[BF16X3 if split else F32]
    scale = "mul" if scale_is_exact(C) else "div"
    N = H8 * W8
    if W8 % 32 == 0 and H8 % 8 == 0 and N % 128 == 0:
        if split and C == 256 and W8 % 64 == 0 and rs_on:
            return ("role-split", 16 if H8 % 16 == 0 else 8, 2 if W8 % 128 == 0 else 1, prec, scale)
        return ("tile", 0, 0, prec, scale)
    return ("generic", 0, 0, prec, scale)


def _corr(B, H8, W8, C, precs, rs_on=True):
    return [dict(B=B, H=H8, W=W8, C=C, prec=p, rs_on=rs_on) for p in precs]


BOTH = (F32, BF16X3)
CORR_CASE_LIST = (
    # generic: N = 459 has ragged 128-row and 256-column tails; 17 x 27 and its level 1 (8 x 13) pool with a dropped row / column
    _corr(3, 17, 27, 256, BOTH) + _corr(1, 16, 24, 256, BOTH) + _corr(1, 24, 40, 256, BOTH)
    + _corr(3, 17, 27, 32, BOTH) + _corr(3, 17, 27, 96, BOTH) + _corr(3, 17, 27, 64, BOTH)
    # fused tile; C = 96 is its true-division epilogue
    + _corr(2, 16, 32, 256, BOTH) + _corr(1, 24, 96, 256, BOTH) + _corr(2, 16, 32, 96, BOTH)
    + _corr(1, 16, 64, 256, (BF16X3,), rs_on=False) + _corr(1, 16, 64, 64, (BF16X3,))
    # role-split: RB 16 / 8, one / two chunks, batch, three one-chunk items per row
    + _corr(1, 16, 64, 256, (BF16X3,)) + _corr(2, 24, 64, 256, (BF16X3,)) + _corr(1, 16, 128, 256, (BF16X3,))
    + _corr(2, 24, 128, 256, (BF16X3,)) + _corr(1, 16, 192, 256, (BF16X3,)))


def corr_name(c):
    return f"{c['B']}x{c['H']}x{c['W']}_c{c['C']}_{PREC[c['prec']]}" + ("" if c["rs_on"] else "_rs0")


CORR_CASES = OrderedDict((corr_name(c), c) for c in CORR_CASE_LIST)


def corr_inputs(c, kind, dev):
    """f1, f2 fp32 [B * N, C], a seed of its own per batch element.  'uniform': [-1, 1); 'spread': a per-channel scale 2^s, s in
    [-6, 3], of its own for each of the two maps, so that a term can be lost relative to the total."""
    B, N, C = c["B"], c["H"] * c["W"], c["C"]
    out = []
    for which in (1, 2):
        rows = []
        for b in range(B):
            gen = torch.Generator().manual_seed(7919 * which + 101 * b + (13 if kind == "spread" else 0))
            x = torch.rand(N, C, generator=gen) * 2 - 1
            if kind == "spread":
                x = x * torch.exp2(torch.rand(C, generator=gen) * 9 - 6)
            rows.append(x)
        out.append(torch.cat(rows).to(dev).contiguous())
    return out


def ref_corr(c, f1, f2):
    """[(ref, bound)] of the four levels, float64 [B, N, N_i] (module docstring)."""
    B, H, W, C = c["B"], c["H"], c["W"], c["C"]
    N = H * W
    a, b = f1.double().view(B, N, C), f2.double().view(B, N, C)
    s = math.sqrt(C)
    v = torch.matmul(a, b.transpose(1, 2)) / s
    A = torch.matmul(a.abs(), b.abs().transpose(1, 2)) / s
    R = torch.matmul(a * a, (b * b).transpose(1, 2)).sqrt() / s
    bnd = two_bounds(c["prec"], C, A, R)
    if not scale_is_exact(C):
        bnd = bnd + 2 * U * (v.abs() + bnd)          # sqrtf(C) rounded once, the quotient rounded once
    levels = [(v, bnd)]
    for i in range(3):
        levels.append(pool_ref(*levels[-1], H >> i, W >> i))
    return levels


def emu_corr(c, f1, f2, levels, mut=None):
    """Torch emulation of the kernels' arithmetic into `levels` ([B * N, N_i] fp32): fp32 accumulation over the 32-channel
    chunks in order; bf16x3 per 16-channel MFMA step as f1_lo f2_hi + f1_hi f2_lo + f1_hi f2_hi (bf16 products are exact in
    fp32).  The scaling is the kernel's (exact multiply or division by sqrtf(C)), the pooling its fp32 window sum.  `mut`: the
    deliberate mistakes of tests/test_mfma_launch_reference.py."""
    B, H, W, C = c["B"], c["H"], c["W"], c["C"]
    N = H * W
    if mut == "batch_f2":                             # every batch element reads batch 0's f2
        f2 = f2.view(B, N, C)[[0] * B].reshape(B * N, C)
    a, b = f1.view(B, N, C), f2.view(B, N, C)
    nC = C - 32 if mut == "drop_chunk" else C
    acc = torch.zeros(B, N, N)
    if c["prec"] == BF16X3:
        ah, al = (t.view(B, N, C) for t in twin_hi_lo(split_ref(f1)))
        bh, bl = (t.view(B, N, C) for t in twin_hi_lo(split_ref(f2)))
        for k in range(0, nC, 16):
            s = slice(k, k + 16)
            if mut != "one_pass":
                if mut != "drop_hilo":
                    acc = acc + torch.matmul(al[..., s], bh[..., s].transpose(1, 2))
                acc = acc + torch.matmul(ah[..., s], bl[..., s].transpose(1, 2))
            acc = acc + torch.matmul(ah[..., s], bh[..., s].transpose(1, 2))
    else:
        for k in range(0, nC, 32):
            acc = acc + torch.matmul(a[..., k:k + 32], b[..., k:k + 32].transpose(1, 2))
    s = torch.tensor(np.sqrt(np.float32(C), dtype=np.float32))
    v = acc * (1.0 / s) if scale_is_exact(C) else acc / s
    if mut == "transpose":
        v = v.transpose(1, 2).contiguous()
    if mut == "tile_shift":                           # the second 32-column target tile, one column to the right
        v = v.clone()
        v[:, :, 32:64] = torch.roll(v[:, :, 32:64], 1, -1)
    levels[0].copy_(v.reshape(B * N, N))
    for i in range(3):
        v = pool_f32(v, H >> i, W >> i, mut if mut in ("pool_offset", "pool_last") else None)
        levels[i + 1].copy_(v.reshape(B * N, -1))


class HipOps:
    """The launches under test on libpriorflow_hip.so."""
    device_kernels = True

    def __init__(self, lib):
        self.lib = lib

    def corr(self, c, f1, f2, levels):
        B, H, W, C = c["B"], c["H"], c["W"], c["C"]
        if c["prec"] == BF16X3:
            tw = [torch.empty(f.shape[0], C // 32, 2, 32, dtype=torch.bfloat16, device=f.device) for f in (f1, f2)]
            self.lib.split_bf16(f1, tw[0])
            self.lib.split_bf16(f2, tw[1])
            self.lib.corr_pyramid_bf16x3(tw[0], tw[1], levels, B, H, W, C)
        else:
            self.lib.corr_pyramid(f1, f2, levels, B, H, W)

    def enc_stem(self, img, w, b, out, twin, relu, stats):
        from prior_flow_amd.engine import pack_stem7x7
        self.lib.debug_dirty_lds(0x7fc00000, like=img)          # every launch behind an LDS full of NaN patterns
        self.lib.enc_stem(img, pack_stem7x7(w), b, out=out, out_split=twin, relu=relu, stats=stats)

    def stem_cap(self):
        """csrc/pf_enc_stem.hip:243: the launch's workgroup cap, two per CU."""
        return 2 * torch.cuda.get_device_properties(0).multi_processor_count


class EmuOps:
    """The same launches on the torch emulations below (device-only kernels); `lib` is the host emulation of the per-element
    entry points.  `mut` names one deliberate mistake."""
    device_kernels = False

    def __init__(self, lib=None, mut=None, cap=3):
        self.lib, self.mut, self.cap = lib, mut, cap

    def corr(self, c, f1, f2, levels):
        emu_corr(c, f1, f2, levels, self.mut)

    def enc_stem(self, img, w, b, out, twin, relu, stats):
        emu_enc_stem(img, w, b, out, twin, relu, stats, self.cap, self.mut)

    def stem_cap(self):
        return self.cap


def run_corr(ops, name, dev, run):
    c = CORR_CASES[name]
    B, H, W, C = c["B"], c["H"], c["W"], c["C"]
    N = H * W
    rs_env = os.environ.get("PRIORFLOW_CORR_RS")
    if (rs_env is not None and rs_env[:1] == "0") == c["rs_on"]:
        run.fails.append(f"corr [{name}]: PRIORFLOW_CORR_RS={rs_env!r} does not select the path this case is for")
        return
    path = corr_select(B, H, W, C, c["prec"] == BF16X3, c["rs_on"])
    kernel = ("corr_pyramid" if c["prec"] == F32 else "split_bf16+corr_pyramid_bf16x3") + ":" + path[0] + \
        (f" RB{path[1]} x{path[2]}" if path[0] == "role-split" else "") + " " + path[4]
    run.paths.add(path)
    for kind in ("uniform", "spread"):
        f1, f2 = corr_inputs(c, kind, dev)
        ref = ref_corr(c, f1, f2)
        outs = []
        for _ in range(2):
            bufs = [guarded(B * N, (H >> i) * (W >> i), dev) for i in range(4)]
            ops.corr(c, f1, f2, [t[0] for t in bufs])
            outs.append(bufs)
        for i, (lv, front, back) in enumerate(outs[0]):
            run.cmp(kernel, f"{kind} level {i}", lv.view(B, N, -1), *ref[i])
            if not (bool(torch.isnan(front).all()) and bool(torch.isnan(back).all())):
                run.fails.append(f"{kernel} [{name}] {kind} level {i}: a guard row was written")
            if not torch.equal(lv.view(torch.int32), outs[1][i][0].view(torch.int32)):
                run.fails.append(f"{kernel} [{name}] {kind} level {i}: two launches on the same inputs differ")
        del ref, outs


# ------------------------------------------------------------------------------------------------------------------------
# family: split  (pf_split_bf16, pf_split_f16 bit for bit) and featpyr (pf_feature_pyramid)
# ------------------------------------------------------------------------------------------------------------------------
SPLIT_ROWS = OrderedDict(one=1, ragged=459, rows=66560)
SPLIT_WIDTHS = (32, 96, 256)


def split_inputs(rows, C, dev, seed):
    """Values over many binades, exact zeros of both signs, bf16- and fp16-representable values (lo == 0), rounding ties, a lo
    that is subnormal in bf16 (|x| ~ 2^-120), fp16 subnormals and values beyond the fp16 range."""
    gen = torch.Generator().manual_seed(seed)
    x = (torch.rand(rows, C, generator=gen) * 2 - 1) * torch.exp2(torch.randint(-20, 12, (rows, C), generator=gen).float())
    sp = torch.tensor([0.0, -0.0, 1.0, -2.5, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11,
                       2.0 ** -120 * (1 + 2.0 ** -10), -2.0 ** -123 * (1 + 2.0 ** -9), 2.0 ** -126, 2.0 ** -130, 6.0e-8, 3.0e-6,
                       65504.0, 65520.0, -7.0e4, 1.0e30, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 0.1])
    n = min(C, sp.numel())
    x[0, :n] = sp[:n]
    x[-1, -n:] = sp[:n]
    return x.to(dev).contiguous()


def run_split(ops, name, dev, run):
    rows = SPLIT_ROWS[name]
    for C in SPLIT_WIDTHS:
        x = split_inputs(rows, C, dev, 31 * C + rows)
        out = torch.full((rows, C // 32, 2, 32), SENT_BF16, dtype=torch.bfloat16, device=dev)
        ops.lib.split_bf16(x, out)
        run.cmp("split_bf16", f"C={C}", out.view(torch.int16).double(), split_ref(x).view(torch.int16).double(), 0.0)
        # fp32 rows with ld_in > C into an f16 map wider than C: the columns past C stay as they were
        whole, view = el.padded(x, C + 8)
        lds = C // 64 + 1
        m = torch.full((rows, lds * 64), SENT_BF16, dtype=torch.float16, device=dev)
        ops.lib.split_f16(view, m)
        run.cmp("split_f16", f"C={C}", m[:, :C].contiguous().view(torch.int16).double(), x.half().view(torch.int16).double(), 0.0)
        if not bool((m[:, C:] == SENT_BF16).all()):
            run.fails.append(f"split_f16 [{name}] C={C}: a column past C was written")
            run.table.add("split_f16", name, float("inf"))
        run.sentinel("split_f16", "input padding", whole[:, C:])


FEAT_SHAPES = OrderedDict(ragged=(3, 17, 27), even=(2, 16, 32))
FEAT_WIDTHS = (256, 100)


def ref_feat(x, B, H, W, C):
    """Levels 1-3 of channel-last rows [B * H * W, C]: (ref, bound) float64 [B * N_i, C]."""
    lv = [(x.double().view(B, H * W, C).transpose(1, 2), torch.zeros(B, C, H * W, dtype=torch.float64, device=x.device))]
    for i in range(3):
        lv.append(pool_ref(*lv[-1], H >> i, W >> i))
    return [(r.transpose(1, 2).reshape(-1, C), b.transpose(1, 2).reshape(-1, C)) for r, b in lv[1:]]


def run_featpyr(ops, name, dev, run):
    B, H, W = FEAT_SHAPES[name]
    for C in FEAT_WIDTHS:
        gen = torch.Generator().manual_seed(5 * C + H)
        x = (torch.rand(B * H * W, C, generator=gen) * 2 - 1).to(dev)
        bufs = [guarded(B * (H >> i) * (W >> i), C, dev) for i in (1, 2, 3)]
        ops.lib.feature_pyramid(x, [t[0] for t in bufs], B, H, W)
        for i, ((lv, front, back), (r, b)) in enumerate(zip(bufs, ref_feat(x, B, H, W, C))):
            run.cmp("feature_pyramid", f"C={C} level {i + 1}", lv, r, b)
            if not (bool(torch.isnan(front).all()) and bool(torch.isnan(back).all())):
                run.fails.append(f"feature_pyramid [{name}] C={C} level {i + 1}: a guard row was written")


# ------------------------------------------------------------------------------------------------------------------------
# family: enc_stem  (pf_enc_stem: fp32 rows, twin, ReLU, fused statistics, persistent workgroups)
# ------------------------------------------------------------------------------------------------------------------------
STEM_K = 147
STEM_SHAPES = OrderedDict(tile=(1, 16, 64), ragged=(2, 18, 70), product=(1, 136, 216), walk=None)


def stem_tiles(Bn, H, W):
    """csrc/pf_enc_stem.hip:237-239: tiles of 8 x 32 output pixels, (per image y, per image x, all)."""
    ty, tx = (H // 2 + 7) // 8, (W // 2 + 31) // 32
    return ty, tx, Bn * ty * tx


def stem_walk_shape(cap):
    """A batch of 250 x 522 images (16 x 9 tiles each, ragged last rows and columns) whose tile count exceeds the launch's
    workgroup cap by more than an image's tiles and is no multiple of it: some workgroups walk a second tile, some do not.
    256 CUs: Bn = 5, 720 tiles over 512 workgroups, 208 of which walk two."""
    H, W = 250, 522
    per = stem_tiles(1, H, W)[2]
    Bn = cap // per + 2
    while Bn * per <= cap or (Bn * per) % cap == 0:
        Bn += 1
    return Bn, H, W


def stem_shape(name, cap):
    """Image sizes (Bn, H, W) of a case; on a small cap (the CPU emulation) the walk case is the ragged shape, 12 tiles."""
    if name != "walk":
        return STEM_SHAPES[name]
    return stem_walk_shape(cap) if cap >= 64 else (2, 18, 70)


def stem_case(shape, dev):
    Bn, H, W = shape
    gen = torch.Generator().manual_seed(17 + H)
    img = (torch.rand(Bn, 3, H, W, generator=gen) * 2 - 1).to(dev)
    w = ((torch.rand(64, 3, 7, 7, generator=gen) * 2 - 1) * 0.2).to(dev)
    b = ((torch.rand(64, generator=gen) * 2 - 1) * 0.3).to(dev)
    return img, w, b


def ref_enc_stem(img, w, b):
    """The 7x7 / 2 pad 3 convolution in float64 over the fp32 image and weights, before the ReLU: (v, bound) [Bn*H2*W2, 64]."""
    Bn, _, H, W = img.shape
    x = img.permute(0, 2, 3, 1).reshape(Bn * H * W, 3)
    r = cl.conv_fp64(x, w, Bn, H // 2, W // 2, 2)
    bb = b.double()[None, :]
    v = r["acc"] + bb
    bnd = two_bounds(BF16X3, STEM_K, r["abs"] + bb.abs(), (r["sq"] + bb * bb).sqrt()) + cl.EPS_EPI * v.abs()
    return v, bnd


def stem_tile_sums(rows, Bn, H2, W2):
    """float64 per-tile sums of stored rows [Bn*H2*W2, 64]: (sum, sum of squares, sum |v|) each [Bn, tiles, 64]."""
    ty, tx = (H2 + 7) // 8, (W2 + 31) // 32
    v = torch.zeros(Bn, ty * 8, tx * 32, 64, dtype=torch.float64, device=rows.device)
    v[:, :H2, :W2] = rows.double().view(Bn, H2, W2, 64)
    t = v.view(Bn, ty, 8, tx, 32, 64)
    f = lambda q: q.sum((2, 4)).reshape(Bn, ty * tx, 64)             # noqa: E731
    return f(t), f(t * t), f(t.abs())


def emu_enc_stem(img, w, b, out, twin, relu, stats, cap, mut=None):
    """Torch emulation of pf_enc_stem: the K axis k = ky * 24 + kx * 3 + c padded to 176, 11 MFMA steps of 16, each
    x_lo w_hi + x_hi w_lo + x_hi w_hi in fp32; bias, ReLU, rows / twin, fp64 statistics per tile.  Tiles are walked as the
    persistent grid does (tile t on workgroup t % cap) so that the mistakes of a second tile can be stated."""
    Bn, _, H, W = img.shape
    H2, W2 = H // 2, W // 2
    xp = torch.nn.functional.pad(img, (3, 3, 3, 3))
    cols = torch.nn.functional.unfold(xp, 7, stride=2).view(Bn, 3, 7, 7, H2 * W2)          # [Bn, c, ky, kx, L]
    xk = torch.zeros(Bn * H2 * W2, 7, 24)
    xk[:, :, :21] = cols.permute(0, 4, 2, 3, 1).reshape(Bn * H2 * W2, 7, 21)
    wk = torch.zeros(64, 7, 24)
    wk[:, :, :21] = w.permute(0, 2, 3, 1).reshape(64, 7, 21)
    xk = torch.cat([xk.reshape(-1, 168), torch.zeros(Bn * H2 * W2, 8)], 1)
    wk = torch.cat([wk.reshape(64, 168), torch.zeros(64, 8)], 1)
    xh = xk.to(torch.bfloat16).float()
    xl = (xk - xh).to(torch.bfloat16).float()
    wh = wk.to(torch.bfloat16).float()
    wl = (wk - wh).to(torch.bfloat16).float()
    acc = torch.zeros(Bn * H2 * W2, 64)
    for k in range(0, 176, 16):
        s = slice(k, k + 16)
        acc = acc + xl[:, s] @ wh[:, s].t()
        acc = acc + xh[:, s] @ wl[:, s].t()
        acc = acc + xh[:, s] @ wh[:, s].t()
    v = acc + b[None, :]
    if relu:
        v = v.clamp_min(0)
    v = v.view(Bn, H2, W2, 64)
    ty, tx, ntiles = stem_tiles(Bn, H, W)
    res = torch.full((Bn, H2, W2, 64), float("nan"))
    if mut == "second_tile":                          # a workgroup's second tile lands on its first tile's rows
        for t in range(ntiles):
            src = t
            dst = t - cap if t >= cap else t
            (si, sy, sx), (di, dy, dx) = ((q // (ty * tx), q // tx % ty * 8, q % tx * 32) for q in (src, dst))
            blk = v[si, sy:sy + 8, sx:sx + 32]
            tgt = res[di, dy:dy + 8, dx:dx + 32]
            hh, ww = min(blk.shape[0], tgt.shape[0]), min(blk.shape[1], tgt.shape[1])
            tgt[:hh, :ww] = blk[:hh, :ww]
    else:
        res = v.clone()
    rows = res.reshape(-1, 64)
    if out is not None:
        out.copy_(rows)
    if twin is not None:
        twin.copy_(split_ref(rows))
    if stats is not None:
        src = rows
        if mut == "stats_last_row" and H2 % 8:         # the partial tiles' last valid row is left out of the sums
            src = res.clone()
            src[:, H2 - 1] = 0
            src = src.reshape(-1, 64)
        s1, s2, _ = stem_tile_sums(src, Bn, H2, W2)
        stats.copy_(torch.stack([s1, s2], -1))


def run_enc_stem(ops, name, dev, run):
    cap = ops.stem_cap()
    shape = stem_shape(name, cap)
    Bn, H, W = shape
    H2, W2 = H // 2, W // 2
    rows = Bn * H2 * W2
    ty, tx, ntiles = stem_tiles(Bn, H, W)
    if name == "walk" and not (ntiles > cap and ntiles % cap):
        run.fails.append(f"enc_stem [walk]: {ntiles} tiles on a cap of {cap} workgroups walk no ragged second trip")
    img, w, b = stem_case(shape, dev)
    v, bnd = ref_enc_stem(img, w, b)
    tag = name
    for relu in (False, True):
        want = v.clamp_min(0) if relu else v
        k = "enc_stem" + ("+relu" if relu else "")
        out, of, ob = guarded(rows, 64, dev)
        tw = torch.full((rows, 2, 2, 32), SENT_BF16, dtype=torch.bfloat16, device=dev)
        st = torch.full((Bn, ty * tx, 64, 2), float("nan"), dtype=torch.float64, device=dev)
        ops.enc_stem(img, w, b, out, tw, relu, st)
        run.cmp(k, "rows", out, want, bnd)
        if not (bool(torch.isnan(of).all()) and bool(torch.isnan(ob).all())):
            run.fails.append(f"{k} [{tag}]: a guard row of the fp32 rows was written")
        if not torch.equal(tw.view(torch.int16), split_ref(out).view(torch.int16)):
            run.fails.append(f"{k} [{tag}]: the twin is not split_bf16 of the rows, bit for bit")
            run.table.add(k + " twin", name, float("inf"))
        s1, s2, sa = stem_tile_sums(out, Bn, H2, W2)
        n = 8 * 32
        run.cmp(k + " stats", "sum", st[..., 0], s1, n * U64 * sa)
        run.cmp(k + " stats", "sum of squares", st[..., 1], s2, n * U64 * s2)
        # rows only / twin only: the same values without the other output
        out2, of2, ob2 = guarded(rows, 64, dev)
        ops.enc_stem(img, w, b, out2, None, relu, None)
        run.cmp(k + " rows only", "rows", out2, want, bnd)
        tw2 = torch.full((rows, 2, 2, 32), SENT_BF16, dtype=torch.bfloat16, device=dev)
        ops.enc_stem(img, w, b, None, tw2, relu, None)
        hi, lo = twin_hi_lo(tw2)
        run.cmp(k + " twin only", "decoded twin", hi.double() + lo.double(), want, bnd + 2.0 ** -16 * (want.abs() + bnd))
        if not cl._is_split(tw2[:, :, 0, :], tw2[:, :, 1, :]):
            run.fails.append(f"{k} [{tag}]: the twin-only output is no hi|lo split")


# ------------------------------------------------------------------------------------------------------------------------
# families: direct  (pf_conv2d_direct, pf_conv2d_direct_group[_f16], pf_conv2d_small) and conf_stem  (pf_conf_stem[_f16])
# ------------------------------------------------------------------------------------------------------------------------
GEOMS = OrderedDict([("2x17x27", (2, 17, 27)), ("2x9x45", (2, 9, 45)), ("1x5x200", (1, 5, 200)), ("1x16x32", (1, 16, 32))])


def direct_select(cin, cout, kh, kw, stride=1, nchw=False, ld_out=4, off_out=0, split=False, rows=True):
    """The kernel pf_direct_conv_dispatch_n takes (csrc/pf_elem_kernels.hip), host logic only:
      :1520-23  the small-Cin limits: LDS of the patch and three weight stages <= 60 KB, ceil(K / 2) <= 160 K pairs,
                KH (31 stride + KW) Cin <= 4096 patch floats, Cin <= 255; beyond them pf_direct_conv_elem (:1560-63)
      :440-443  stem7x7c2_ok: 7x7, Cin 2, stride 1, channel-last, Cout % 64 == 0, rows 16-byte aligned (ld_out, off_out % 4),
                a twin at off_out % 8 == 0
      :1540-54  such a stem with Cout == 128 is pf_flow_stem_kernel (bf16x3), any other pf_stem7x7c2_valu (fp32)
      :1556-58  everything else inside the limits is pf_small_conv_mfma, fp32 rows only"""
    K = kh * kw * cin
    lds = (kh * (31 * stride + kw) * (cin | 1) + 4 + 3 * 16 * 64) * 4
    if lds <= 60 * 1024 and (K + 1) // 2 <= 160 and kh * (31 * stride + kw) * cin <= 16 * 256 and cin <= 255:
        if (kh == 7 and kw == 7 and cin == 2 and stride == 1 and not nchw and cout % 64 == 0
                and (not rows or (ld_out % 4 == 0 and off_out % 4 == 0)) and (not split or off_out % 8 == 0)):
            return "pf_flow_stem_kernel" if cout == 128 else "pf_stem7x7c2_valu"
        return None if (split or not rows) else "pf_small_conv_mfma"
    return "pf_direct_conv_elem"


DIRECT_PREC = {"pf_flow_stem_kernel": BF16X3, "pf_stem7x7c2_valu": F32, "pf_small_conv_mfma": F32, "pf_direct_conv_elem": F32}
# (entry, cin, cout, k, stride, nchw, kernel)
DIRECT_LAYERS = (("direct", 2, 128, 7, 1, False, "pf_flow_stem_kernel"), ("direct", 2, 64, 7, 1, False, "pf_stem7x7c2_valu"),
                 ("direct", 2, 192, 7, 1, False, "pf_stem7x7c2_valu"), ("direct", 8, 32, 3, 1, False, "pf_small_conv_mfma"),
                 ("direct", 32, 16, 3, 1, False, "pf_small_conv_mfma"), ("small", 8, 32, 3, 2, False, "pf_small_conv_mfma"),
                 ("small", 3, 64, 7, 1, True, "pf_small_conv_mfma"), ("small", 3, 64, 7, 2, True, "pf_small_conv_mfma"),
                 ("direct", 96, 32, 3, 1, False, "pf_direct_conv_elem"))


def pack_direct(w):
    """[Cout, Cin, KH, KW] -> [KH * KW][Cin][Cout] (engine.pack_direct)."""
    cout, cin, kh, kw = w.shape
    return w.permute(2, 3, 1, 0).reshape(kh * kw, cin, cout).contiguous()


def conv_ref(x, w, b, prec, B, H, W, stride, in_bound=None):
    """float64 convolution of channel-last rows x with bias, before the ReLU: (v, bound).  in_bound: a bound on x's own error,
    which enters as sum |w| in_bound."""
    cout, cin, kh, kw = w.shape
    r = cl.conv_fp64(x, w, B, H, W, stride)
    bb = b.double()[None, :]
    v = r["acc"] + bb
    bnd = two_bounds(prec, kh * kw * cin, r["abs"] + bb.abs(), (r["sq"] + bb * bb).sqrt()) + cl.EPS_EPI * v.abs()
    if in_bound is not None:
        bnd = bnd + cl.conv_fp64(in_bound, w.abs(), B, H, W, stride, terms=("acc",))["acc"]
    return v, bnd


def _layer_data(gen, cin, cout, k, rows_in, dev):
    x = cl._rand_inputs(gen, rows_in, cin, "cpu").to(dev)
    w = (torch.randn(cout, cin, k, k, generator=gen) / math.sqrt(cin * k * k)).to(dev)
    b = (torch.rand(cout, generator=gen) - 0.5).to(dev)
    return x, w, b


def _check_rows(run, kernel, what, whole, off, cout, want, bnd):
    run.cmp(kernel, what, whole[:, off:off + cout], want, bnd)
    run.sentinel(kernel, what + " beside the slice", el.outside(whole, off, cout))


def _check_form(run, kernel, what, form, off, cout, rows32, want, bnd):
    """A twin / f16 map written at column `off`: bit-equal to the split / .half() of the fp32 rows when both were written, else its
    decoded values with conv_launches' representation term; every other column still the sentinel."""
    f16 = form.dtype == torch.float16
    if f16:
        got, mask = form[:, off:off + cout], torch.ones(form.shape[1], dtype=torch.bool, device=form.device)
        mask[off:off + cout] = False
        clean = bool((form[:, mask] == SENT_BF16).all())
        same = rows32 is None or torch.equal(got, rows32.half())
        val, rep = got.double(), 2.0 ** -11 * (want.abs() + bnd) + 2.0 ** -25
    else:
        hi, lo = twin_hi_lo(form)
        mask = torch.ones(hi.shape[1], dtype=torch.bool, device=form.device)
        mask[off:off + cout] = False
        clean = bool((hi[:, mask] == SENT_BF16).all()) and bool((lo[:, mask] == SENT_BF16).all())
        same = rows32 is None or (torch.equal(hi[:, off:off + cout], rows32.to(torch.bfloat16).float())
                                  and torch.equal(lo[:, off:off + cout], (rows32 - rows32.to(torch.bfloat16).float()).to(torch.bfloat16).float()))
        val, rep = hi[:, off:off + cout].double() + lo[:, off:off + cout].double(), 2.0 ** -16 * (want.abs() + bnd)
    if not clean:
        run.fails.append(f"{kernel} [{run.shape}] {what}: written outside its columns")
    if not same:
        run.fails.append(f"{kernel} [{run.shape}] {what}: not the split / fp16 rounding of the fp32 rows, bit for bit")
    if not (clean and same):
        run.table.add(kernel, run.shape, float("inf"))
    if rows32 is None:
        run.cmp(kernel, what + " decoded", val, want, bnd + rep)


def _form_buf(kind, rows, width, dev):
    if kind == "f16":
        return torch.full((rows, (width + 63) // 64 * 64), SENT_BF16, dtype=torch.float16, device=dev)
    return torch.full((rows, (width + 31) // 32, 2, 32), SENT_BF16, dtype=torch.bfloat16, device=dev)


def run_direct(ops, name, dev, run):
    B, H, W = GEOMS[name]
    lib = ops.lib
    for li, (entry, cin, cout, k, stride, nchw, kernel) in enumerate(DIRECT_LAYERS):
        gen = torch.Generator().manual_seed(1000 * li + H)
        rows, rows_in = B * H * W, B * H * stride * W * stride
        off_in, ld_in, off_out, ld_out = 4, cin + 8, 8, cout + 16
        got = direct_select(cin, cout, k, k, stride, nchw, ld_out, off_out)
        if got != kernel:
            run.fails.append(f"direct [{name}]: {k}x{k}/{stride} {cin}->{cout} dispatches to {got}, the case is for {kernel}")
            continue
        prec = DIRECT_PREC[kernel]
        tag = kernel if ops.device_kernels else kernel + " (host)"
        x, w, b = _layer_data(gen, cin, cout, k, rows_in, dev)
        v, bnd = conv_ref(x, w, b, prec, B, H, W, stride)
        wp = pack_direct(w)
        for relu in (False, True):
            want = v.clamp_min(0) if relu else v
            what = f"{k}x{k}/{stride} {cin}->{cout}" + (" relu" if relu else "")
            out = torch.full((rows, ld_out), SENT_F32, device=dev)
            if nchw:
                xin = x.view(B, H * stride, W * stride, cin).permute(0, 3, 1, 2).contiguous()
                lib.conv2d_small(xin, True, 0, cin, wp, b, out, off_out, cout, k, k, stride, relu, B, H, W)
            else:
                xin, _ = el.padded(x, ld_in, off_in)
                if entry == "small":
                    lib.conv2d_small(xin, False, off_in, cin, wp, b, out, off_out, cout, k, k, stride, relu, B, H, W)
                else:
                    lib.conv2d_direct(xin, off_in, cin, wp, b, out, off_out, cout, k, k, relu, B, H, W)
            _check_rows(run, tag, what, out, off_out, cout, want, bnd)
    # group launches of the 7x7 2 -> C stems: 1, 3 and 4 problems with inputs and weights of their own; rows + twin, twin only,
    # f16 map only and rows + f16 map
    for cout, kernel in ((128, "pf_flow_stem_kernel"), (64, "pf_stem7x7c2_valu")):
        prec = DIRECT_PREC[kernel]
        tag = (kernel if ops.device_kernels else kernel + " (host)") + " group"
        rows = B * H * W
        for n, form, with_rows in ((1, "twin", True), (3, "twin", False), (4, "f16", False), (3, "f16", True)):
            if direct_select(2, cout, 7, 7, 1, False, cout + 16, 8, True, with_rows) != kernel:
                run.fails.append(f"direct [{name}]: the {n}-problem group of 2->{cout} stems does not dispatch to {kernel}")
                continue
            probs, refs = [], []
            for i in range(n):
                gen = torch.Generator().manual_seed(77 * n + i + cout)
                x, w, b = _layer_data(gen, 2, cout, 7, rows, dev)
                xin, _ = el.padded(x, 8, 4)
                out = torch.full((rows, cout + 16), SENT_F32, device=dev) if with_rows else None
                fb = _form_buf(form, rows, cout + 16, dev)
                probs.append((xin, 4, pack_direct(w), b, out, 8, fb))
                refs.append(conv_ref(x, w, b, prec, B, H, W, 1))
            lib.conv2d_direct_group(probs, 2, cout, 7, 7, True, B, H, W)
            for i, (p, (v, bnd)) in enumerate(zip(probs, refs)):
                want = v.clamp_min(0)
                what = f"{n} problems, problem {i}, {form}" + ("+rows" if with_rows else " only")
                if with_rows:
                    _check_rows(run, tag, what, p[4], 8, cout, want, bnd)
                _check_form(run, tag, what, p[6], 8, cout, p[4][:, 8:8 + cout] if with_rows else None, want, bnd)


def ref_conf_stem(x, w1, b1, w2, b2, B, H, W):
    """relu(conv3x3(relu(conv3x3(x)))) in float64, both layers fp32 (K = 72, 288).  The first layer's bound enters the second as
    sum |w2| bound1; ReLU is 1-Lipschitz, so nothing is excluded."""
    v1, bnd1 = conv_ref(x, w1, b1, F32, B, H, W, 1)
    v2, bnd2 = conv_ref(v1.clamp_min(0), w2, b2, F32, B, H, W, 1, in_bound=bnd1)
    return v2.clamp_min(0), bnd2


def emu_conf_stem(x, w1, b1, w2, b2, B, H, W, mut=None):
    """fp32 torch statement of pf_conf_stem; mut 'no_relu': the intermediate map without its ReLU."""
    nchw = x.view(B, H, W, -1).permute(0, 3, 1, 2)
    m = torch.nn.functional.conv2d(nchw, w1, b1, padding=1)
    if mut != "no_relu":
        m = m.clamp_min(0)
    return torch.nn.functional.conv2d(m, w2, b2, padding=1).clamp_min(0).permute(0, 2, 3, 1).reshape(B * H * W, -1)


def conf_case(name, dev):
    B, H, W = GEOMS[name]
    gen = torch.Generator().manual_seed(41 + W)
    x, w1, b1 = _layer_data(gen, 8, 32, 3, B * H * W, dev)
    _, w2, b2 = _layer_data(gen, 32, 16, 3, 1, dev)
    return x, w1, b1, w2, b2


def run_conf_stem(ops, name, dev, run):
    B, H, W = GEOMS[name]
    rows = B * H * W
    x, w1, b1, w2, b2 = conf_case(name, dev)
    want, bnd = ref_conf_stem(x, w1, b1, w2, b2, B, H, W)
    xin, _ = el.padded(x, 20, 4)
    p1, p2 = pack_direct(w1), pack_direct(w2)
    k = "conf_stem" if ops.device_kernels else "conf_stem (host)"
    for form, with_rows in ((None, True), ("twin", True), ("twin", False), ("f16", True), ("f16", False)):
        out = torch.full((rows, 40), SENT_F32, device=dev) if with_rows else None
        fb = _form_buf(form, rows, 40, dev) if form else None
        ops.lib.conf_stem(xin, 4, p1, b1, p2, b2, out, 8, B, H, W, out_split=fb)
        what = (form or "rows") + ("+rows" if form and with_rows else "")
        if with_rows:
            _check_rows(run, k, what, out, 8, 16, want, bnd)
        if form:
            _check_form(run, k + ("_f16" if form == "f16" else ""), what, fb, 8, 16, out[:, 8:24] if with_rows else None, want, bnd)


def emu_flow_stem(x, w, b, B, H, W, relu=True, mut=None):
    """Torch emulation of pf_flow_stem_kernel's arithmetic (device-only): the 7x7 2 -> C convolution as bf16x3 over the 98
    products in steps of 16, x_lo w_hi + x_hi w_lo + x_hi w_hi in fp32.  mut 'top_tap': at the top border (output row 0) the tap
    row that reads input row 0 is dropped."""
    cout = w.shape[0]
    nchw = torch.nn.functional.pad(x.view(B, H, W, 2).permute(0, 3, 1, 2), (3, 3, 3, 3))
    cols = torch.nn.functional.unfold(nchw, 7).view(B, 2, 7, 7, H, W).clone()          # [B, c, ky, kx, y, x]
    if mut == "top_tap":
        cols[:, :, 3, :, 0, :] = 0
    xk = torch.zeros(B * H * W, 112)
    xk[:, :98] = cols.permute(0, 4, 5, 2, 3, 1).reshape(B * H * W, 98)
    wk = torch.zeros(cout, 112)
    wk[:, :98] = w.permute(0, 2, 3, 1).reshape(cout, 98)
    xh, wh = xk.to(torch.bfloat16).float(), wk.to(torch.bfloat16).float()
    xl, wl = (xk - xh).to(torch.bfloat16).float(), (wk - wh).to(torch.bfloat16).float()
    acc = torch.zeros(B * H * W, cout)
    for k in range(0, 112, 16):
        q = slice(k, k + 16)
        acc = acc + xl[:, q] @ wh[:, q].t()
        acc = acc + xh[:, q] @ wl[:, q].t()
        acc = acc + xh[:, q] @ wh[:, q].t()
    v = acc + b[None, :]
    return v.clamp_min(0) if relu else v


# ------------------------------------------------------------------------------------------------------------------------
# family: combine_conv  (pf_dccl_combine_conv1x1 and its _f16 form: rotate back + add + 1x1 324 -> 256 bf16x3 + ReLU)
# ------------------------------------------------------------------------------------------------------------------------
COMBINE_SHAPES = ("even", "ragged")            # elem_launches.SHAPES: (2, 16, 32) and (3, 17, 27)


def combine_conv_case(shape, kind, group, dev):
    c = el.combine_case(shape, dev, kind, seed=20 + group)
    gen = torch.Generator().manual_seed(300 + group)
    c["w"] = (torch.randn(256, el.CORR_CH, 1, 1, generator=gen) / math.sqrt(el.CORR_CH)).to(dev)
    c["b"] = (torch.rand(256, generator=gen) - 0.5).to(dev)
    return c


def ref_combine_conv(c, mut=None):
    """The combined row and its bound from elem_launches.ref_combine, then the 1x1 convolution in float64: K = 324, bf16x3; the
    combined row's bound enters as the input perturbation sum |w| bound."""
    row, rb = el.ref_combine(c)["out"]
    v, bnd = conv_ref(row, c["w"], c["b"], BF16X3, c["B"], c["H"], c["W"], 1, in_bound=rb)
    return v.clamp_min(0), bnd


def emu_combine_conv(lib, c):
    """Torch emulation (device-only kernel): the combined fp32 row from the host emulation's pf_dccl_combine, then the bf16x3
    products over the 324 (352 padded) channels in steps of 16."""
    R = c["R"]
    row = torch.empty(R, el.CORR_CH)
    lib.dccl_combine(c["own"], c["raw"], c["g_back"], row, c["B"], c["H"], c["W"])
    xk, wk = torch.zeros(R, 352), torch.zeros(256, 352)
    xk[:, :el.CORR_CH], wk[:, :el.CORR_CH] = row, c["w"].view(256, el.CORR_CH)
    xh, wh = xk.to(torch.bfloat16).float(), wk.to(torch.bfloat16).float()
    xl, wl = (xk - xh).to(torch.bfloat16).float(), (wk - wh).to(torch.bfloat16).float()
    acc = torch.zeros(R, 256)
    for k in range(0, 352, 16):
        q = slice(k, k + 16)
        acc = acc + xl[:, q] @ wh[:, q].t()
        acc = acc + xh[:, q] @ wl[:, q].t()
        acc = acc + xh[:, q] @ wh[:, q].t()
    return (acc + c["b"][None, :]).clamp_min(0)


def run_combine_conv(ops, shape, dev, run):
    from prior_flow_amd._lib import PREC_BF16X3
    from prior_flow_amd.engine import Conv, pack_mfma
    k = "dccl_combine_conv1x1" if ops.device_kernels else "dccl_combine_conv1x1 (torch)"
    for kind in ("real", "tearing"):
        cs = [combine_conv_case(shape, "real" if kind == "real" else "random", g, dev) for g in range(2)]
        refs = [ref_combine_conv(c) for c in cs]
        R = cs[0]["R"]
        B, H, W = cs[0]["B"], cs[0]["H"], cs[0]["W"]
        if not ops.device_kernels:
            for c, (want, bnd) in zip(cs, refs):
                run.cmp(k, f"{kind} rows", emu_combine_conv(ops.lib, c), want, bnd)
            continue
        convs = [Conv(*pack_mfma(c["w"], c["b"]), 1, 1, el.CORR_CH, 256, PREC_BF16X3) for c in cs]
        for n, form, with_rows in ((1, None, True), (2, None, True), (2, "twin", True), (1, "twin", False), (2, "f16", True), (1, "f16", False)):
            items, bufs = [], []                      # a twin / map needs off_out % 32 == 0: the slice sits at column 32 of 320
            for c, cv in list(zip(cs, convs))[:n]:
                own, _ = el.padded(c["own"], 336)
                raw, _ = el.padded(c["raw"], 336)
                out = torch.full((R, 320), SENT_F32, device=dev) if with_rows else None
                fb = _form_buf(form, R, 320, dev) if form else None
                items.append((own, raw, c["g_back"], cv, out, 32) + ((fb,) if form else ()))
                bufs.append((out, fb))
            ops.lib.dccl_combine_conv1x1(items, B, H, W)
            for i, ((out, fb), (want, bnd)) in enumerate(zip(bufs, refs)):
                what = f"{kind} {n} groups, group {i}, " + (form or "rows") + ("+rows" if form and with_rows else "")
                if with_rows:
                    _check_rows(run, k, what, out, 32, 256, want, bnd)
                if form:
                    _check_form(run, k + ("_f16" if form == "f16" else ""), what, fb, 32, 256, out[:, 32:288] if with_rows else None, want, bnd)


# ------------------------------------------------------------------------------------------------------------------------
# the case table
# ------------------------------------------------------------------------------------------------------------------------
FAMILIES = OrderedDict(
    corr=(run_corr, tuple(CORR_CASES)),
    split=(run_split, tuple(SPLIT_ROWS)),
    featpyr=(run_featpyr, tuple(FEAT_SHAPES)),
    enc_stem=(run_enc_stem, tuple(STEM_SHAPES)),
    direct=(run_direct, tuple(GEOMS)),
    conf_stem=(run_conf_stem, tuple(GEOMS)),
    combine_conv=(run_combine_conv, COMBINE_SHAPES),
)
CASES = [(fam, shape) for fam, (_, shapes) in FAMILIES.items() for shape in shapes]


def cases(device_type):
    return list(CASES)


def case_env(family, shape):
    """Environment a case needs set before its launches ({} for most): PRIORFLOW_CORR_RS is read per launch."""
    if family == "corr" and not CORR_CASES[shape]["rs_on"]:
        return {"PRIORFLOW_CORR_RS": "0"}
    return {}


class PathRun(Run):
    def __init__(self, table, shape, paths):
        super().__init__(table, shape)
        self.paths = paths


def run_case(lib, family, shape, dev, table, paths=None):
    """Runs one (family, shape) case on `lib` (a PfLib, or EmuOps); returns the list of failures (empty = pass).  `paths` collects
    the corr paths taken.  A case that left no row in the table is a failure."""
    ops = lib if hasattr(lib, "device_kernels") else HipOps(lib)
    run = PathRun(table, shape, paths if paths is not None else set())
    before = len(table.rows)
    FAMILIES[family][0](ops, shape, dev, run)
    if len(table.rows) == before and not run.fails:
        run.fails.append(f"{family} [{shape}]: nothing was compared")
    return run.fails


def selectable_corr_paths():
    """Every (path, RB, chunks, precision, scale branch) corr_launch can select, by sweeping corr_select over map sizes, widths,
    both operand forms and both settings of the switch."""
    out = set()
    for H8 in range(16, 49):
        for W8 in list(range(16, 72)) + [96, 128, 192, 256]:
            for C in (32, 64, 96, 256):
                for split in (False, True):
                    for rs_on in (True, False):
                        out.add(corr_select(1, H8, W8, C, split, rs_on))
    out.discard(None)
    return out
