"""Float64 restatement of the alternate_corr lookups (pf_feature_pyramid + pf_dccl_lookup_feat) for the tests.

The geometry -- coordinates, wrap, zero padding, the cross view's level-0 grid sample -- is the oracle's own fp32 code
(priorflow_oracle.cycle_bilinear_sampler), so every tap lands where the kernels put it; only the VALUES are float64: the
pooled features, the correlation rows <f1[n], P_i(f2)[p]> / sqrt(C) and the bilinear sums.  With ``absolute=True`` the
same lookup runs on |f1| and |f2|: sum_j w_j sum_c |f1 P_i(f2)| / sqrt(C), the magnitude an error bound scales with.
Works on any device and on a subset of pixels (4K geometry: a few hundred sampled rows).
"""
import math

import torch

import priorflow_oracle as po


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
