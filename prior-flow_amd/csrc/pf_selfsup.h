// Self-supervised criterion on unlabelled 360-degree video: a spherical photometric term through the model's
// cyclic sampler and a first-order edge-aware smoothness term, with their gradient with respect to every prediction.  This header
// is the statement: the device kernel (pf_selfsup.hip) and the host emulation (tests/emu/pf_emu_selfsup.cpp) compile it, and
// tests/selfsup_ref.py restates it in float64.  Every step is one rounded fp32 operation (-ffp-contract=off).
//
// One branch: n predictions f_i = (u, v) [B,2,H,W] in pixels, image1 / image2 [B,3,H,W] (0..255), weight [H*W] (the solid-angle
// weight uniform_loss uses), mask [B,H,W] bytes or NULL, i_weights[n], Z = B * sum weight (computed by the caller).
//
//   bad(p)      = !(|u| < max_flow) || !(|v| < max_flow)                  NaN, +-inf and over-range alike
//   photometric = weight(p) * (1/3) sum_c rho_p(d_c) / Z,  d_c = (image2_c sampled at (x + u, y + v) - image1_c(p)) / 255,
//                 rho_p(d) = sqrt(d^2 + eps_photo^2); the taps are pf_wraptaps', the mix pf_wrapmix's (the bits pf_cycle_warp
//                 writes).  Left out (zero loss, zero gradient) when mask(p) != 0 or bad(p): a bad flow is replaced by zero before
//                 any tap is computed, and the pixel's terms are deselected afterwards.
//   d/du, d/dv  = rho_p'(d_c) / 255 times the derivative of pf_wrapmix in the two fractions, from the four tap values:
//                 dI/dx = (1 - yw)(c - a) + yw (d - b), dI/dy = (1 - xw)(b - a) + xw (d - c), the four factors taken from the tap
//                 weights (1 - yw = wa + wc, yw = wb + wd, 1 - xw = wa + wb, xw = wc + wd).  Where y clamps, b == a and d == c.
//   smoothness  = pairs (p, p_r), p_r = ((x + 1) mod W, y), every x (the seam is a pair like any other), coefficient
//                 weight(p) e_h(p), and (p, p_d), p_d = (x, y + 1), only for y + 1 < H, coefficient (weight(p) + weight(p_d)) / 2
//                 * e_v(p); e = exp(-edge_lambda (1/3) sum_c |image1_c(q) - image1_c(p)| / 255); a pair costs
//                 coefficient * (rho_s(du) + rho_s(dv)) / Z, rho_s(d) = sqrt(d^2 + eps_smooth^2), du = u(q) - u(p) (plain: the
//                 predictions do not wrap).  Not masked.  A pair with a bad end is left out.
//   gradient    = a gather: a pixel sums the up to four pairs it belongs to, in the fixed order right, left, down, up.
//   grads[i]    = i_weights[i] * (w_photo * d photo + w_smooth * d smooth); every element is written.
//   partials    = double [n][B][nblk][4] = {photo, smooth, sum of weight over the pixels the photometric term used, count of bad
//                 pixels} per chunk; the caller adds the chunks (the two-stage sum of pf_seq_loss).
//
// How the fp32 steps are spelled (the restatement's bounds cover them): the divisions by Z are made once per pixel and per pair, on
// weight(p) and on the pair coefficients, not once per prediction; / 255 and / 3 of the per-prediction part are multiplications
// by the rounded reciprocals; with x = d^2 + eps^2, rho = x * rsq(x) and rho' = d * rsq(x), rsq one v_rsq_f32 on the device.
//
// A thread owns ONE pixel, so the lanes of a wave read consecutive floats of a row.  Chunk k holds pixels [k * chunk, (k + 1) *
// chunk) of the H * W, chunk = ceil(H * W / nblk) (pf_ss_chunk): the cut depends on nblk alone.  (Four consecutive pixels per
// thread, sharing the row's flow through registers, were built first and dropped: the lanes then stand 16 bytes apart and every
// load and tap instruction touches 8 or 9 cache lines where it now touches 2 or 3 -- DESIGN.md section 21: 2.1x the time.)  Every
// index is a pixel index below H * W: x is wrapped or below W, y clamped by pf_wraptaps or tested against H; nothing is indexed
// by a flow value that has not passed bad().
#pragma once
#include "pf_elem.h"

constexpr int PF_SS_MAX = 32;            // terms of one launch
constexpr int PF_SS_SUMS = 4;
constexpr int PF_SS_MAX_NBLK = 4096;
constexpr int PF_SS_MAX_GRID = 65536;

struct PfSelfSupArgs {
    const float* pred[PF_SS_MAX]; float* grad[PF_SS_MAX]; float i_weight[PF_SS_MAX];
    const float* image1; const float* image2; const float* weight; const unsigned char* mask;
    double* partials;                    // [n][B][nblk][4]
    int n, B, H, W, nblk;
    float w_photo, w_smooth, eps_photo, eps_smooth, edge_lambda, max_flow, z;
};

PF_HD long pf_ss_chunk(int H, int W, int nblk) { return ((long)H * W + nblk - 1) / nblk; }      // pixels of a chunk

PF_HD bool pf_ss_bad(float u, float v, float max_flow) { return !(fabsf(u) < max_flow) || !(fabsf(v) < max_flow); }

// e of the pair (p, q) from the three channels of image1 at both ends
PF_HD float pf_ss_edge(float p0, float p1, float p2, float q0, float q1, float q2, float edge_lambda) {
    float s = fabsf(q0 - p0) + fabsf(q1 - p1);
    s = s + fabsf(q2 - p2);
    const float m = (s / 3.f) / 255.f;
    return expf(-(edge_lambda * m));
}
// 1 / sqrt(x) for x > 0: one v_rsq_f32 (1 ulp) on the device, a division and a square root on the host.  rho(d) = x * rsq(x) and
// rho'(d) = d * rsq(x) with x = d^2 + eps^2 then cost one transcendental instead of a correctly rounded square root and division.
PF_HD float pf_ss_rsq(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_rsqf(x);
#else
    return 1.f / sqrtf(x);
#endif
}
constexpr float PF_SS_INV255 = 1.f / 255.f, PF_SS_THIRD = 1.f / 3.f;
// one pair with coefficient c (already divided by Z): its loss, and its derivative with respect to the FAR end's (u, v) (the near
// end's is the negative)
PF_HD void pf_ss_pair(float c, float du, float dv, float eps, float& loss, float& gu, float& gv) {
    const float xu = du * du + eps * eps, xv = dv * dv + eps * eps;
    const float ru = pf_ss_rsq(xu), rv = pf_ss_rsq(xv);
    loss = c * (xu * ru + xv * rv);
    gu = c * (du * ru);
    gv = c * (dv * rv);
}

// photometric term of one pixel at a flow that passed the leave-out test (or was replaced by zero): loss, d loss / du, d loss / dv;
// wz = weight / Z
PF_HD void pf_ss_photo(const PfSelfSupArgs& a, const float* im2, int x, int y, float u, float v, float i1_0, float i1_1, float i1_2,
                       float wz, float& loss, float& gu, float& gv) {
    const long N = (long)a.H * a.W;
    const PfWrapTaps t = pf_wraptaps((float)x + u, (float)y + v, a.H, a.W);
    const float omy = t.wa + t.wc, yw = t.wb + t.wd, omx = t.wa + t.wb, xw = t.wc + t.wd;
    const float i1[3] = {i1_0, i1_1, i1_2};
    const float e2 = a.eps_photo * a.eps_photo;
    float s = 0.f, su = 0.f, sv = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* p = im2 + c * N;
        const float ta = p[t.ia], tb = p[t.ib], tc = p[t.ic], td = p[t.id];
        const float d = (pf_wrapmix(t, ta, tb, tc, td) - i1[c]) * PF_SS_INV255;
        const float xx = d * d + e2;
        const float r = pf_ss_rsq(xx);
        const float q = (d * r) * PF_SS_INV255;
        const float dx = omy * (tc - ta) + yw * (td - tb);
        const float dy = omx * (tb - ta) + xw * (td - tc);
        s = s + xx * r;
        su = su + q * dx;
        sv = sv + q * dy;
    }
    loss = wz * (s * PF_SS_THIRD);
    gu = wz * (su * PF_SS_THIRD);
    gv = wz * (sv * PF_SS_THIRD);
}

// what the n predictions share at one pixel: image1, weight / Z, mask and the four pair coefficients (divided by Z)
struct PfSsCtx {
    int x, y, xl, xr;                    // the pixel and the columns of its left and right neighbours (wrapped)
    int dn, up;                          // row offsets of the neighbour rows: W and -W, 0 where there is none (the load stays in the image)
    float i1[3];
    float w, wz;
    bool masked;
    float cl, cr, cd, cu;                // pairs (p_l, p), (p, p_r), (p, p_d), (p_u, p); cd / cu are 0 where there is no such row
};

PF_HD void pf_ss_context(const PfSelfSupArgs& a, long b, long pix, PfSsCtx& c) {
    const int W = a.W;
    const long N = (long)a.H * W;
    c.y = (int)(pix / W);
    c.x = (int)(pix - (long)c.y * W);
    c.xl = c.x == 0 ? W - 1 : c.x - 1;
    c.xr = c.x + 1 == W ? 0 : c.x + 1;
    c.up = c.y > 0 ? -W : 0; c.dn = c.y + 1 < a.H ? W : 0;
    const long row = (long)c.y * W, n = row + c.x, nl = row + c.xl, nr = row + c.xr, md = n + c.dn, mu = n + c.up;
    const float* i1 = a.image1 + b * 3 * N;
    float l[3], r[3], d[3], u[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        l[ch] = i1[ch * N + nl]; c.i1[ch] = i1[ch * N + n]; r[ch] = i1[ch * N + nr];
        d[ch] = i1[ch * N + md]; u[ch] = i1[ch * N + mu];
    }
    c.w = a.weight[n];
    c.wz = c.w / a.z;
    c.masked = a.mask ? a.mask[b * N + n] != 0 : false;
    c.cl = (a.weight[nl] * pf_ss_edge(l[0], l[1], l[2], c.i1[0], c.i1[1], c.i1[2], a.edge_lambda)) / a.z;
    c.cr = (c.w * pf_ss_edge(c.i1[0], c.i1[1], c.i1[2], r[0], r[1], r[2], a.edge_lambda)) / a.z;
    const float ed = pf_ss_edge(c.i1[0], c.i1[1], c.i1[2], d[0], d[1], d[2], a.edge_lambda);
    const float eu = pf_ss_edge(u[0], u[1], u[2], c.i1[0], c.i1[1], c.i1[2], a.edge_lambda);
    c.cd = c.dn ? (((c.w + a.weight[md]) * 0.5f) * ed) / a.z : 0.f;
    c.cu = c.up ? (((a.weight[mu] + c.w) * 0.5f) * eu) / a.z : 0.f;
}

// prediction i at one pixel: writes the pixel's two gradient elements, adds its share to sums[4].  Written without branches around
// loads: a flow that fails the test is replaced by zero BEFORE anything is computed from it, every load is at a pixel of the
// image, and what must not count is deselected at the end -- so all loads of the pixel are in flight together.
PF_HD void pf_ss_term(const PfSelfSupArgs& a, const PfSsCtx& c, long b, int i, double (&sums)[PF_SS_SUMS]) {
    const int W = a.W;
    const long N = (long)a.H * W, row = (long)c.y * W, n = row + c.x;
    const float* pu = a.pred[i] + b * 2 * N;
    const float* pv = pu + N;
    float* g = a.grad[i] ? a.grad[i] + b * 2 * N : nullptr;
    float uj = pu[n], vj = pv[n], ul = pu[row + c.xl], vl = pv[row + c.xl], ur = pu[row + c.xr], vr = pv[row + c.xr];
    float ud = pu[n + c.dn], vd = pv[n + c.dn], uu = pu[n + c.up], vu = pv[n + c.up];
    const bool okj = !pf_ss_bad(uj, vj, a.max_flow), used = okj && !c.masked;
    const bool okl = okj && !pf_ss_bad(ul, vl, a.max_flow), okr = okj && !pf_ss_bad(ur, vr, a.max_flow);
    const bool okd = okj && c.dn != 0 && !pf_ss_bad(ud, vd, a.max_flow), oku = okj && c.up != 0 && !pf_ss_bad(uu, vu, a.max_flow);
    uj = okj ? uj : 0.f; vj = okj ? vj : 0.f;
    ul = okl ? ul : 0.f; vl = okl ? vl : 0.f; ur = okr ? ur : 0.f; vr = okr ? vr : 0.f;
    ud = okd ? ud : 0.f; vd = okd ? vd : 0.f; uu = oku ? uu : 0.f; vu = oku ? vu : 0.f;
    float pl, pgu, pgv;
    pf_ss_photo(a, a.image2 + b * 3 * N, c.x, c.y, uj, vj, c.i1[0], c.i1[1], c.i1[2], c.wz, pl, pgu, pgv);
    pl = used ? pl : 0.f; pgu = used ? pgu : 0.f; pgv = used ? pgv : 0.f;
    float lr, ld, t, gu, gv, su = 0.f, sv = 0.f;
    pf_ss_pair(c.cr, ur - uj, vr - vj, a.eps_smooth, lr, gu, gv);                              // (p, p_r): this pixel's own
    su = su - (okr ? gu : 0.f); sv = sv - (okr ? gv : 0.f);
    pf_ss_pair(c.cl, uj - ul, vj - vl, a.eps_smooth, t, gu, gv);                               // (p_l, p)
    su = su + (okl ? gu : 0.f); sv = sv + (okl ? gv : 0.f);
    pf_ss_pair(c.cd, ud - uj, vd - vj, a.eps_smooth, ld, gu, gv);                              // (p, p_d): this pixel's own
    su = su - (okd ? gu : 0.f); sv = sv - (okd ? gv : 0.f);
    pf_ss_pair(c.cu, uj - uu, vj - vu, a.eps_smooth, t, gu, gv);                               // (p_u, p)
    su = su + (oku ? gu : 0.f); sv = sv + (oku ? gv : 0.f);
    sums[0] += (double)pl;
    sums[1] += (double)(okr ? lr : 0.f);
    sums[1] += (double)(okd ? ld : 0.f);
    sums[2] += used ? (double)c.w : 0.0;
    sums[3] += okj ? 0.0 : 1.0;
    if (g) {
        g[n] = a.i_weight[i] * (a.w_photo * pgu + a.w_smooth * su);
        g[N + n] = a.i_weight[i] * (a.w_photo * pgv + a.w_smooth * sv);
    }
}

static inline bool pf_ss_finite(float x) { return x - x == 0.f; }
// do the byte ranges [p, p + np) and [q, q + nq) meet?  (NULL meets nothing)
static inline bool pf_ss_meet(const void* p, size_t np, const void* q, size_t nq) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return p && q && a < b + nq && b < a + np;
}

// the argument checks of pf_selfsup_loss_batch and the fill of its argument block (host; shared with the emulation)
static inline int pf_selfsup_check(const float* const* preds, const float* image1, const float* image2, const float* weight,
                                   const unsigned char* mask, const float* i_weights, float* const* grads, double* partials, int nblk,
                                   int n, int B, int H, int W, float w_photo, float w_smooth, float eps_photo, float eps_smooth,
                                   float edge_lambda, float max_flow, float z, int blocks, PfSelfSupArgs& a) {
    if (!preds || !image1 || !image2 || !weight || !i_weights || !partials || ((uintptr_t)partials & 7)) return PF_ERR_BAD_ARG;
    if (B < 1 || H < 2 || W < 2 || (long)H * W >= (1L << 30) || n < 1 || n > PF_SS_MAX || nblk < 1 || nblk > PF_SS_MAX_NBLK)
        return PF_ERR_BAD_SHAPE;
    if (blocks < 0 || blocks > PF_SS_MAX_GRID) return PF_ERR_BAD_ARG;
    // eps * eps must not underflow (rho(0) = eps^2 * rsq(eps^2)), max_flow must be finite (a flow that passes is squared)
    if (!(pf_ss_finite(w_photo) && pf_ss_finite(w_smooth) && pf_ss_finite(eps_photo) && eps_photo * eps_photo > 0.f
          && pf_ss_finite(eps_smooth) && eps_smooth * eps_smooth > 0.f && eps_photo > 0.f && eps_smooth > 0.f && edge_lambda >= 0.f
          && pf_ss_finite(edge_lambda) && max_flow > 0.f && pf_ss_finite(max_flow) && z > 0.f && pf_ss_finite(z)))
        return PF_ERR_BAD_ARG;
    // no output may meet an input or another output, as byte ranges
    const size_t N = (size_t)H * W, nflow = (size_t)B * 2 * N * 4, npart = (size_t)n * B * nblk * PF_SS_SUMS * 8;
    const void* ins[4] = {image1, image2, weight, mask};
    const size_t nins[4] = {(size_t)B * 3 * N * 4, (size_t)B * 3 * N * 4, N * 4, (size_t)B * N};
    for (int k = 0; k < 4; ++k)
        if (pf_ss_meet(ins[k], nins[k], partials, npart)) return PF_ERR_BAD_ARG;
    for (int i = 0; i < n; ++i) {
        if (!preds[i] || pf_ss_meet(preds[i], nflow, partials, npart)) return PF_ERR_BAD_ARG;
        const float* gi = grads ? grads[i] : nullptr;
        if (!gi) continue;
        if (pf_ss_meet(gi, nflow, partials, npart)) return PF_ERR_BAD_ARG;
        for (int k = 0; k < 4; ++k)
            if (pf_ss_meet(gi, nflow, ins[k], nins[k])) return PF_ERR_BAD_ARG;
        for (int m = 0; m < n; ++m)
            if (pf_ss_meet(gi, nflow, preds[m], nflow) || (m < i && pf_ss_meet(gi, nflow, grads[m], nflow))) return PF_ERR_BAD_ARG;
    }
    for (int i = 0; i < PF_SS_MAX; ++i) {
        const int j = i < n ? i : 0;
        a.pred[i] = preds[j]; a.grad[i] = grads ? grads[j] : nullptr; a.i_weight[i] = i_weights[j];
    }
    a.image1 = image1; a.image2 = image2; a.weight = weight; a.mask = mask; a.partials = partials;
    a.n = n; a.B = B; a.H = H; a.W = W; a.nblk = nblk;
    a.w_photo = w_photo; a.w_smooth = w_smooth; a.eps_photo = eps_photo; a.eps_smooth = eps_smooth; a.edge_lambda = edge_lambda;
    a.max_flow = max_flow; a.z = z;
    return PF_OK;
}
