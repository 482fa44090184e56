"""Float64 restatement of the alternate_corr lookups (pf_feature_pyramid + pf_dccl_lookup_feat) for the tests.

The geometry -- coordinates, wrap, zero padding, the cross view's level-0 grid sample -- is the oracle's own fp32 code
(priorflow_oracle.cycle_bilinear_sampler), so every tap lands where the kernels put it; only the VALUES are float64: the
pooled features, the correlation rows <f1[n], P_i(f2)[p]> / sqrt(C) and the bilinear sums.  With ``absolute=True`` the
same lookup runs on |f1| and |f2|: sum_j w_j sum_c |f1 P_i(f2)| / sqrt(C), the magnitude an error bound scales with.
Works on any device and on a subset of pixels (4K geometry: a few hundred sampled rows).

The bound of one output value (``bound``), following tests/elem_launches.py: K terms summed in any order are off by at most
(K + 1) U sum |term|, U = 2^-24.  The geometry is shared with the kernels bit for bit, so the four weights carry no error and
only the roundings of the values count, each relative to a term of sum_j w_j sum_c |f1 P_i(f2)| / sqrt(C):
  * C      products of one dot product (FMA or product + addition, sequential in a lane or a butterfly over the wave);
  * 3 x 5  the pooling levels below the corner: (((a + b) + c) + d) * 0.25, counted as four additions and a scale each
           (P_i(|f2|) >= |P_i(f2)|, so the magnitude with pooled absolute values covers every partial sum);
  * 1      the product with a.scale = 1 / sqrt(C) (the fp32 value of the scale itself is inside the + 1);
  * 4      the bilinear sum: the product with the weight and the three additions.
K_TERMS(C) = C + 20, i.e. 24 U ... 533 U for C = 4 ... 512 (K_FEAT = 32 eps = 64 U of tests/test_hip_alt_corr.py is the count
of the pixel path's butterfly at C = 256 alone).  Random signs stay far below it: a sum of C terms of either sign is off by
about sqrt(C) U rms, so ratios of 0.01 to 0.1 are that gap and not slack in the count.

The path decision (``corners``, ``units``): pf_taps2_corners restated on the same fp32 geometry gives the element index of every
corner with a weight per (pixel, level, view); the bounding box of a 2 x 4 pixel tile's corners is the window pf_lookup_feat_kernel
stages, nwin its element count, and nwin <= LF_CAP the tile path.
"""
import math

import torch

import priorflow_oracle as po

U = 2.0 ** -24
LF_TY, LF_TX, LF_CAP = 2, 4, 192          # csrc/pf_lookup.hip: pixel tile of a workgroup, rows of the LDS window


def k_terms(C: int) -> int:
    """Roundings per output value of pf_dccl_lookup_feat (see the module docstring)."""
    return C + 3 * 5 + 1 + 4


def bound(C: int, mag: torch.Tensor) -> torch.Tensor:
    """(K + 1) U sum |term| on the ``absolute=True`` magnitude."""
    return (k_terms(C) + 1) * U * mag


def pool_levels(f2: torch.Tensor):
    """[f2, P(f2), P^2(f2), P^3(f2)]: 2x2 means with avg_pool2d floor semantics (odd sizes drop the last row / column)."""
    out = [f2]
    for _ in range(3):
        c = out[-1]
        h, w = c.shape[-2] // 2, c.shape[-1] // 2
        c = c[..., : 2 * h, : 2 * w]
        out.append((c[..., 0::2, 0::2] + c[..., 0::2, 1::2] + c[..., 1::2, 0::2] + c[..., 1::2, 1::2]) * 0.25)
    return out


def rows(x: torch.Tensor) -> torch.Tensor:
    """[B, C, H, W] -> channel-last rows [B*H*W, C]."""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


def lookup_feat(coords, f1_own, f2_own, f1_oth, f2_oth, g_w2c, pix=None, absolute=False):
    """(own, raw) [len(pix), 324] float64 as pf_dccl_lookup_feat writes them (channel = level*81 + a*9 + b).

    coords [B,2,H,W] fp32; f* [B,C,H,W]; g_w2c [2,H,W] fp32; pix: flat rows b*N + n (default: all)."""
    B, C, H, W = f1_own.shape
    N = H * W
    dev = f1_own.device
    pix = torch.arange(B * N, device=dev) if pix is None else pix.to(dev)
    P = pix.numel()
    b, n = pix // N, pix % N
    prep = (lambda t: t.double().abs()) if absolute else (lambda t: t.double())  # noqa: E731
    d = torch.linspace(-4, 4, 9, device=dev)
    off_x = d.view(9, 1).expand(9, 9).reshape(1, 81)            # slow axis a -> x
    off_y = d.view(1, 9).expand(9, 9).reshape(1, 81)
    c = coords.to(dev)
    cx0 = c[:, 0].reshape(B, N)[b, n].unsqueeze(1)
    cy0 = c[:, 1].reshape(B, N)[b, n].unsqueeze(1)
    a_own = prep(f1_own).permute(0, 2, 3, 1).reshape(B, N, C)[b, n]
    a_oth = prep(f1_oth).permute(0, 2, 3, 1).reshape(B, N, C)[b, n]
    lv_own, lv_oth = pool_levels(prep(f2_own)), pool_levels(prep(f2_oth))
    gw = g_w2c.to(dev)[None].expand(P, -1, -1, -1)
    scale = 1.0 / math.sqrt(C)

    def volume_rows(a, lv):                                     # [P, 1, h, w]: row n of level i's volume
        h, w = lv.shape[-2:]
        out = torch.empty(P, h * w, dtype=torch.float64, device=dev)
        for bb in range(B):
            m = b == bb
            if bool(m.any()):
                out[m] = (a[m] @ lv[bb].reshape(C, h * w)) * scale
        return out.view(P, 1, h, w)

    own_l, raw_l = [], []
    for i in range(4):
        cx = cx0 / 2 ** i + off_x
        cy = cy0 / 2 ** i + off_y
        own_l.append(po.cycle_bilinear_sampler(volume_rows(a_own, lv_own[i]), cx, cy)[:, 0])
        g = po.cycle_bilinear_sampler(gw, cx, cy)               # level-i coordinates into the LEVEL-0 grid
        raw_l.append(po.cycle_bilinear_sampler(volume_rows(a_oth, lv_oth[i]), g[:, 0], g[:, 1])[:, 0])
    return torch.cat(own_l, 1), torch.cat(raw_l, 1)


def _tap_corners(x, y, H, W):
    """pf_taps0v + pf_taps2_corners on fp32 positions (x already wrapped): the element index y * W + x of the four corners nw, ne,
    sw, se [..., 4] (-1 where the weight is 0, as the kernel's dedup sees it) and their fp32 weights."""
    ix, iy = po._roundtrip(x, W), po._roundtrip(y, H)
    fx, fy = torch.floor(ix), torch.floor(iy)
    wx, wy = ix - fx, iy - fy
    ex, ey = 1 - wx, 1 - wy
    idx, wgt = [], []
    for dy, dx, w in ((0, 0, ey * ex), (0, 1, ey * wx), (1, 0, wy * ex), (1, 1, wy * wx)):
        xi, yi = fx + dx, fy + dy
        ok = (xi >= 0) & (xi <= W - 1) & (yi >= 0) & (yi <= H - 1)
        w = torch.where(ok, w, torch.zeros_like(w))
        e = (yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1)).long()
        idx.append(torch.where(w != 0, e, torch.full_like(e, -1)))
        wgt.append(w)
    return torch.stack(idx, -1), torch.stack(wgt, -1)


def corners(coords, g_w2c):
    """pf_lookup_feat_tap + pf_taps2_corners for every (pixel, level, view): a list over the levels of dicts with
    ``own`` / ``raw`` = (idx [B*N, 81, 4] element indices into the level's H_i x W_i map, -1 where the weight is 0; weights fp32) and
    ``pos`` = the fp32 positions handed to pf_taps0v: own-view taps, grid taps (level-0 size) and what the grid sample returns."""
    B, _, H, W = coords.shape
    N = H * W
    d = torch.linspace(-4, 4, 9)
    off_x = d.view(9, 1).expand(9, 9).reshape(1, 81)
    off_y = d.view(1, 9).expand(9, 9).reshape(1, 81)
    cx0 = coords[:, 0].reshape(B * N, 1)
    cy0 = coords[:, 1].reshape(B * N, 1)
    gw = g_w2c[None].expand(B * N, -1, -1, -1)
    out = []
    for i in range(4):
        Hl, Wl = H >> i, W >> i
        cx = cx0 / 2 ** i + off_x
        cy = cy0 / 2 ** i + off_y
        xo, xg = po.pymod(cx, Wl), po.pymod(cx, W)
        g = po.bilin0(gw, xg, cy)
        xc, gy = po.pymod(g[:, 0], Wl), g[:, 1]
        out.append(dict(own=_tap_corners(xo, cy, Hl, Wl), raw=_tap_corners(xc, gy, Hl, Wl),
                        pos=dict(own=(xo, cy), grid=(xg, cy), raw=(xc, gy))))
    return out


def tile_of_pixel(B, H, W):
    """[B*N] the workgroup (blockIdx.x) that owns each pixel, and the number of tiles."""
    ty, tx = (H + LF_TY - 1) // LF_TY, (W + LF_TX - 1) // LF_TX
    n = torch.arange(H * W)
    t = (n // W // LF_TY) * tx + (n % W) // LF_TX
    return (torch.arange(B).view(B, 1) * (ty * tx) + t.view(1, -1)).reshape(-1), B * ty * tx


def tile_boxes(idx, Wl, tile, T):
    """idx [B*N, K] element indices (-1: none) -> per tile (ymin, ymax, xmin, xmax) and nwin (0 where the tile has no corner)."""
    big = 1 << 30
    ok = idx >= 0
    y, x = torch.div(idx, Wl, rounding_mode="floor"), idx % Wl
    red = lambda v, fill, how: torch.full((T,), fill, dtype=torch.long).scatter_reduce(       # noqa: E731
        0, tile, getattr(torch.where(ok, v, torch.full_like(v, fill)), how)(1), how)
    y0, y1, x0, x1 = red(y, big, "amin"), red(y, -1, "amax"), red(x, big, "amin"), red(x, -1, "amax")
    nwin = torch.where(y1 >= y0, (y1 - y0 + 1) * (x1 - x0 + 1), torch.zeros_like(y0))
    return (y0, y1, x0, x1), nwin


def units(corn, B, H, W):
    """nwin [tiles, 4 levels, 2 views (own, cross)] of one launch, and the path counts the kernel must report:
    [#units with nwin <= LF_CAP, #units with nwin > LF_CAP]."""
    tile, T = tile_of_pixel(B, H, W)
    nwin = torch.zeros(T, 4, 2, dtype=torch.long)
    for i, lv in enumerate(corn):
        for v, key in enumerate(("own", "raw")):
            nwin[:, i, v] = tile_boxes(lv[key][0].reshape(B * H * W, -1), W >> i, tile, T)[1]
    return nwin, [int((nwin <= LF_CAP).sum()), int((nwin > LF_CAP).sum())]
