"""Float64 numpy statement of the self-supervised criterion, written from the definition and not from the
kernel.  Not collected; imported by tests/test_selfsup_host.py and tests/test_hip_selfsup.py.

One branch: n predictions f_i = (u, v) [B,2,H,W] in pixels, image1 / image2 [B,3,H,W] in 0..255, weight [H*W], mask [B,H,W] bytes
or None, i_weights[n], Z = B * sum weight.
  bad(p)   = not (|u| < max_flow and |v| < max_flow)                           NaN, +-inf and over-range alike
  photo    = sum over pixels with mask == 0 and not bad of weight(p) (1/3) sum_c rho(d_c, eps_photo) / Z,
             d_c = (I2w_c - image1_c(p)) / 255, I2w_c = image2_c at (x + u, y + v): x wraps (Python modulo), y clamps, bilinear
             with the weights of the unclamped fractions
  smooth   = sum over pairs (p, p_r), p_r = ((x + 1) mod W, y), of weight(p) e (rho(du, eps_smooth) + rho(dv, eps_smooth)) / Z
             + sum over pairs (p, p_d), p_d = (x, y + 1), y + 1 < H, of (weight(p) + weight(p_d)) / 2 e (...) / Z,
             e = exp(-edge_lambda (1/3) sum_c |image1_c(q) - image1_c(p)| / 255), du = u(q) - u(p); a pair with a bad end is left out
  rho(d, eps) = sqrt(d^2 + eps^2)
  loss_i   = w_photo photo_i + w_smooth smooth_i,  grads[i] = i_weights[i] d loss_i / d f_i (analytic, below)

Every function takes `fault`: None, or the name of one deliberate mistake (FAULTS) that tests/test_selfsup_host.py builds into a
copy of the statement to show that the cases notice it.

The bounds (U = 2^-24; OPS = 64 U covers the rounded fp32 operations of any one chain below, none of which has 64):
  the sampling position x + u is rounded once and reduced modulo W: dx = U (|x + u| + W); y + v once: dy = U |y + v|.
  I2w: |dI/dx| dx + |dI/dy| dy + OPS max|tap|;  d: that / 255 + OPS;  rho: |rho'| <= 1, so d's error + OPS rho.
  photo of a pixel: weight / Z (mean_c of rho's error) + OPS photo.
  rho'(d) / 255 = d / rho / 255 has slope eps^2 / rho^3 (<= 1 / eps at d = 0): (d's error eps^2 / rho^3 + OPS) / 255.
  dI/dx = (1 - yw)(c - a) + yw (d - b): |(d - b) - (c - a)| (dy + OPS) + OPS (|c - a| + |d - b|); dI/dy likewise with dx.
  a pair's coefficient w e: relative OPS (1 + edge_lambda m), m the mean absolute difference / 255 (the exponent's error is
  absolute in e's logarithm); its loss and its gradient c du / rho (slope eps^2 / rho^3 times U |du| <= U |du / rho|): relative
  that + OPS.
  a gradient element: i_weight (w_photo photo's + w_smooth sum of its pairs') + OPS of its magnitude.
A pixel whose fp64 sampling fraction lies within dx (dy) of an integer, and not on it, may take other taps in fp32 (`near`); a
fraction exactly on an integer comes from an integer sum, which fp32 holds exactly.

Finite differences (fd_check): the loss is a sum of local terms -- photo(p), the pair to the right and the pair below, owned by p --
so pixels three apart (the columns beyond the last multiple of three on their own, because of the seam) share none, and one
perturbed evaluation differentiates a whole colour class.  Between the kinks of the sampler I2w is linear in u, so the third
derivative of a term is rho''' times the cube of the inner slope, |rho'''| <= 0.86 / eps^2 (at d = eps / 2):
  tolerance = h^2 / 6 (weight / Z (1/3) sum_c 0.86 / eps_photo^2 |slope_c / 255|^3 w_photo
              + w_smooth sum over the pixel's pairs of c 0.86 / eps_smooth^2 / Z) + 16 * 2^-52 sum |terms touched| / h.
"""
from dataclasses import dataclass

import numpy as np

U = 2.0 ** -24
OPS = 64 * U
RHO3 = 0.86                      # max |rho'''| eps^2
FAULTS = ("weight_dropped", "mask_ignored", "grad_swapped", "seam_clamped", "last_row_pair", "i_weights_reversed",
          "edges_from_image2", "vertical_weight_p_only", "no_255_in_grad")


@dataclass
class Params:
    w_photo: float = 1.0
    w_smooth: float = 2.0
    eps_photo: float = 0.01
    eps_smooth: float = 0.001
    edge_lambda: float = 150.0
    max_flow: float = 400.0


def z_of(weight, B):
    return float(B) * float(np.asarray(weight, np.float64).sum())


def rho(d, eps):
    return np.sqrt(d * d + eps * eps)


def term(f, image1, image2, weight, mask, prm, fault=None):
    """One prediction.  Returns a dict: photo, smooth, used, left_out (totals); gu, gv [B,H,W] = d (w_photo photo + w_smooth smooth)
    / d (u, v); own [B,H,W] = the terms each pixel owns (w_photo, w_smooth applied); and the bounds e_photo, e_smooth (totals),
    e_gu, e_gv, e_own, near [B,H,W], fd3_u, fd3_v (third-derivative bounds of fd_check)."""
    f = np.asarray(f, np.float64)
    i1, i2 = np.asarray(image1, np.float64), np.asarray(image2, np.float64)
    B, _, H, W = f.shape
    w = np.asarray(weight, np.float64).reshape(H, W)
    Z = z_of(weight, B)
    if fault == "weight_dropped":
        w = np.full_like(w, 1.0 / (H * W))
    u, v = f[:, 0], f[:, 1]
    with np.errstate(invalid="ignore"):
        bad = ~(np.abs(u) < prm.max_flow) | ~(np.abs(v) < prm.max_flow)
    masked = np.zeros((B, H, W), bool) if mask is None or fault == "mask_ignored" else np.asarray(mask) != 0
    used = ~bad & ~masked
    us, vs = np.where(bad, 0.0, u), np.where(bad, 0.0, v)
    Y, X = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    # ---- photometric
    gx, gy = np.mod(X + us, W), Y + vs
    fx, fy = np.floor(gx), np.floor(gy)
    xw, yw = gx - fx, gy - fy
    x0 = fx.astype(np.int64) % W
    x1 = (x0 + 1) % W
    y0 = np.clip(fy, 0, H - 1).astype(np.int64)
    y1 = np.clip(fy + 1, 0, H - 1).astype(np.int64)
    bi = np.arange(B)[:, None, None, None]
    ci = np.arange(3)[None, :, None, None]
    ta, tb = i2[bi, ci, y0[:, None], x0[:, None]], i2[bi, ci, y1[:, None], x0[:, None]]
    tc, td = i2[bi, ci, y0[:, None], x1[:, None]], i2[bi, ci, y1[:, None], x1[:, None]]
    xw_, yw_ = xw[:, None], yw[:, None]
    I = (1 - xw_) * (1 - yw_) * ta + (1 - xw_) * yw_ * tb + xw_ * (1 - yw_) * tc + xw_ * yw_ * td
    dIx = (1 - yw_) * (tc - ta) + yw_ * (td - tb)
    dIy = (1 - xw_) * (tb - ta) + xw_ * (td - tc)
    d = (I - i1) / 255.0
    r = rho(d, prm.eps_photo)
    q = d / r if fault == "no_255_in_grad" else d / r / 255.0
    wz = (w / Z)[None]
    photo_px = np.where(used, wz * r.mean(1), 0.0)
    pgu = np.where(used, wz * (q * dIx).mean(1), 0.0)
    pgv = np.where(used, wz * (q * dIy).mean(1), 0.0)
    # bounds of the photometric part
    dxp = (U * (np.abs(X + us) + W))[:, None]
    dyp = (U * np.abs(Y + vs))[:, None]
    tmax = np.maximum(np.maximum(np.abs(ta), np.abs(tb)), np.maximum(np.abs(tc), np.abs(td)))
    e_d = (np.abs(dIx) * dxp + np.abs(dIy) * dyp + OPS * tmax) / 255.0 + OPS
    e_r = e_d + OPS * r
    e_photo_px = np.where(used, wz * e_r.mean(1) + OPS * photo_px, 0.0)
    e_q = (e_d * prm.eps_photo ** 2 / r ** 3 + OPS) / 255.0
    cross = np.abs((td - tb) - (tc - ta))
    e_dx = cross * (dyp + OPS) + OPS * (np.abs(tc - ta) + np.abs(td - tb))
    e_dy = cross * (dxp + OPS) + OPS * (np.abs(tb - ta) + np.abs(td - tc))
    e_pgu = np.where(used, wz * ((e_q * np.abs(dIx) + np.abs(q) * e_dx).mean(1) + OPS * np.abs(q * dIx).mean(1)), 0.0)
    e_pgv = np.where(used, wz * ((e_q * np.abs(dIy) + np.abs(q) * e_dy).mean(1) + OPS * np.abs(q * dIy).mean(1)), 0.0)
    distx, disty = np.minimum(xw, 1 - xw), np.minimum(yw, 1 - yw)
    near = used & (((distx > 0) & (distx <= dxp[:, 0])) | ((disty > 0) & (disty <= dyp[:, 0])))
    kink = np.minimum(distx, disty)
    fd3_u = np.where(used, wz * (RHO3 / prm.eps_photo ** 2 * np.abs(dIx / 255.0) ** 3).mean(1), 0.0) * prm.w_photo
    fd3_v = np.where(used, wz * (RHO3 / prm.eps_photo ** 2 * np.abs(dIy / 255.0) ** 3).mean(1), 0.0) * prm.w_photo
    # ---- smoothness
    ie = i2 if fault == "edges_from_image2" else i1
    gsu, gsv = np.zeros((B, H, W)), np.zeros((B, H, W))
    e_gs, abs_gs = np.zeros((B, H, W)), np.zeros((B, H, W))
    smooth_px, e_smooth_px = np.zeros((B, H, W)), np.zeros((B, H, W))
    fd3_s = np.zeros((B, H, W))
    xr = np.minimum(np.arange(W) + 1, W - 1) if fault == "seam_clamped" else (np.arange(W) + 1) % W
    rows = H if fault == "last_row_pair" else H - 1
    yd = np.minimum(np.arange(rows) + 1, H - 1)
    for axis in ("h", "v"):
        if axis == "h":
            sl, far = (slice(None), slice(None), slice(None)), (slice(None), slice(None), xr)
            ie_far, wpair = ie[:, :, :, xr], w
        else:
            sl, far = (slice(None), slice(0, rows), slice(None)), (slice(None), yd, slice(None))
            ie_far = ie[:, :, yd, :]
            wpair = w[:rows] if fault == "vertical_weight_p_only" else 0.5 * (w[:rows] + w[yd])
        m = np.abs(ie_far - ie[(slice(None),) + sl]).mean(1) / 255.0
        c = wpair[None] * np.exp(-prm.edge_lambda * m)
        ok = ~bad[sl] & ~bad[far]
        du = np.where(ok, us[far] - us[sl], 0.0)
        dv = np.where(ok, vs[far] - vs[sl], 0.0)
        ru, rv = rho(du, prm.eps_smooth), rho(dv, prm.eps_smooth)
        pl = np.where(ok, c * (ru + rv) / Z, 0.0)
        fu, fv = np.where(ok, c * du / ru / Z, 0.0), np.where(ok, c * dv / rv / Z, 0.0)       # w.r.t. the far end
        rel = OPS * (1 + prm.edge_lambda * m) + OPS
        smooth_px[sl] += pl
        e_smooth_px[sl] += pl * rel
        t3 = np.where(ok, c * RHO3 / prm.eps_smooth ** 2 / Z, 0.0)
        for acc, val in ((gsu, fu), (gsv, fv)):
            acc[sl] -= val
            np.add.at(acc, far, val)
        for acc, val in ((e_gs, np.where(ok, c / Z, 0.0) * rel), (abs_gs, np.abs(fu) + np.abs(fv)), (fd3_s, t3)):
            acc[sl] += val
            np.add.at(acc, far, val)
    gu = prm.w_photo * pgu + prm.w_smooth * gsu
    gv = prm.w_photo * pgv + prm.w_smooth * gsv
    if fault == "grad_swapped":
        gu, gv = gv, gu
    e_gu = abs(prm.w_photo) * e_pgu + abs(prm.w_smooth) * e_gs + OPS * (np.abs(prm.w_photo * pgu) + abs(prm.w_smooth) * abs_gs)
    e_gv = abs(prm.w_photo) * e_pgv + abs(prm.w_smooth) * e_gs + OPS * (np.abs(prm.w_photo * pgv) + abs(prm.w_smooth) * abs_gs)
    return dict(photo=photo_px.sum(), smooth=smooth_px.sum(), used=np.where(used, w[None], 0.0).sum(), left_out=int(bad.sum()),
                gu=gu, gv=gv, own=prm.w_photo * photo_px + prm.w_smooth * smooth_px,
                e_photo=e_photo_px.sum(), e_smooth=e_smooth_px.sum(), e_gu=e_gu, e_gv=e_gv, near=near, kink=kink, bad=bad, sampled=used,
                fd3_u=fd3_u + prm.w_smooth * fd3_s, fd3_v=fd3_v + prm.w_smooth * fd3_s)


def criterion(preds, image1, image2, weight, mask, i_weights, prm=Params(), fault=None):
    """All n predictions: a list of term() dicts, each with grads [B,2,H,W] = i_weights[i] * (gu, gv) and its bound e_grads."""
    n = len(preds)
    out = []
    for i, f in enumerate(preds):
        t = term(f, image1, image2, weight, mask, prm, fault)
        iw = float(i_weights[n - 1 - i] if fault == "i_weights_reversed" else i_weights[i])
        t["grads"] = iw * np.stack([t["gu"], t["gv"]], 1)
        t["e_grads"] = abs(iw) * np.stack([t["e_gu"], t["e_gv"]], 1) + OPS * np.abs(t["grads"])
        t["loss"] = prm.w_photo * t["photo"] + prm.w_smooth * t["smooth"]
        out.append(t)
    return out


def colours(H, W):
    """[H,W] colour classes: two pixels of one class share no term of the loss (three apart; the columns past the last multiple of
    three are classes of their own, so that the seam joins no two of a class)."""
    main = 3 * (W // 3)
    cx = np.where(np.arange(W) < main, np.arange(W) % 3, 3 + np.arange(W) - main)
    cy = np.arange(H) % 3
    return cy[:, None] * 5 + cx[None, :]


def fd_check(f, image1, image2, weight, mask, prm=Params(), h=1e-6, kink=1e-3):
    """Central differences of the statement's own loss against its analytic gradient, per element.  Returns (worst ratio of the
    difference to the tolerance over the elements kept, share of the pixels excluded for a sampling fraction within `kink` of an
    integer)."""
    f = np.asarray(f, np.float64)
    B, _, H, W = f.shape
    base = term(f, image1, image2, weight, mask, prm)
    col = colours(H, W)
    keep = ~base["bad"] & (~base["sampled"] | (base["kink"] > kink))
    worst = 0.0

    def gathered(m):                      # the terms a pixel touches: its own, its left neighbour's, the one above's
        out = m + np.roll(m, 1, axis=2)
        out[:, 1:] += m[:, :-1]
        return out

    for k in np.unique(col):
        sel = (col == k)[None] & np.ones((B, 1, 1), bool)
        for comp, key, k3 in ((0, "gu", "fd3_u"), (1, "gv", "fd3_v")):
            fp, fm = f.copy(), f.copy()
            fp[:, comp][sel] += h
            fm[:, comp][sel] -= h
            op, om = term(fp, image1, image2, weight, mask, prm)["own"], term(fm, image1, image2, weight, mask, prm)["own"]
            num = gathered(op - om) / (2 * h)
            tol = h * h / 6 * base[k3] + 16 * 2.0 ** -52 * gathered(np.abs(op) + np.abs(om)) / h
            pick = sel & keep
            if pick.any():
                worst = max(worst, float((np.abs(num - base[key])[pick] / tol[pick]).max()))
    return worst, 1.0 - keep.sum() / max(1, (~base["bad"]).sum())
