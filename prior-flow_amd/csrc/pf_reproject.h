// Depth along the trajectory: rigid reprojection of an inverse-depth panorama into the next camera, a z-tested forward splat and
// a per-pixel recursive depth filter (include/priorflow_hip.h: pf_reproj_project, pf_zsplat_front,
// pf_zsplat_accumulate, pf_zsplat_resolve, pf_depth_update).  The statement, once, for the device kernels (pf_reproject.hip), the
// host emulation (tests/emu/pf_emu_reproject.cpp) and the C checks.  The bearings, pf_vp_erp and the point-motion convention are
// pf_epipolar.h's, the scales, the quantiser, the direct sink, the hole rule and the column-wrap / pole-row-drop tap rule are
// pf_splat.h's; nothing of them is restated here.
//
// Convention (section 20): a scene point X in the earlier frame's axes is R X + T in the later frame's; T [B,3] lies in DEVICE
// memory, in the unit of the inverse depth d (T = baseline t).
//
// Project, source pixel (x, y) of image b, every step a rounded fp32 operation (the units are built without contraction):
//   p = pf_ego_p(x, ...),   s = R p + d T,   n = |s| (n = 1 when T is the zero vector: a camera that did not move changes no
//   depth, bit for bit),   d' = d / n,   (qx, qy) = pf_vp_erp(s),   u = qx - x wrapped into [-W/2, W/2),   v = qy - y
//   (u = v = 0 when T is the zero vector and R the identity matrix, bit for bit: the same camera sees every point where it was)
//   LEFT OUT when the mask byte is set, !(weight > 0), !(0 <= d < 2^30) or !(n >= n_min) (a NaN compares false): flow 0, d' = 0,
//   valid = 0.  d = 0, a point at infinity, is legal: it moves by the rotation alone and keeps d' = 0.  Nothing is indexed by an
//   input value.
//
// Z-tested splat of the STORED fp32 flow, d', weight, valid and C = 0..4 payload planes; no transcendental from here on, so the
// device, the emulation and an fp32 restatement agree bit for bit.  A source pixel COUNTS when valid != 0, weight > 0,
// 0 <= d' < 2^30, the landing point q = (x + u, y + v) is nearer than 2^30 and every payload value is (|value| < 2^30; a NaN
// compares false).  Its taps are section 18's: x0 = floor(qx), columns x0, x0 + 1 wrapped, rows y0, y0 + 1 dropped outside the
// map, b_k the bilinear weights; a tap is USED when b_k >= b_min.
//   front:       front[p] = max(front[p], bits(d')) over the used taps, as 32-bit unsigned integers.  d' >= +0 (a -0 is read as
//                +0), so the order of the bit patterns is the order of the values; a max commutes.  All-zero before the call.
//   accumulate:  the same taps again; a tap counts iff d' ztol >= front[p] as floats (ztol = 2^tol_log2, computed once on the
//                host; front = 0 admits everything).  With w_n = min(weight, w_max) / w_max:
//                  N_c[p] += (w_n b_k) clamp(src_c, +-vmax)   planes 0 .. C - 1        scale fn
//                  N_d[p] += (w_n b_k) min(d', dmax)          plane C                  scale fn
//                  D[p]   += w_n b_k                          plane C + 1              scale fd
//                  cov[p] += b_k                              plane C + 2              scale fd
//                64-bit integers, a contribution pf_splat_quant(value, scale), scales = pf_splat_scales(1, H, W, max(dmax, vmax)):
//                w_n <= 1 and a pixel's b_k sum to at most 1, so section 18's bound holds and the adds commute.
//   resolve:     hole = cov < cmin or D <= 0 (pf_splat_is_hole); d_out = N_d / D, w_out = w_max D / cov, out_c = N_c / D; a hole
//                gives 0, 0, 0 and hole byte 1.  Zeros are written over every sum and over front: all-zero again after a call.
//
// Update, per pixel, in place on the state (d_s, w_s) with a measurement (d_m, w_m, disagree), Odometry's flags [B,4] and the
// filter's own seg [B] (int32).  A weight above w_max is read as w_max.  A side counts when its weight is positive and finite and
// 0 <= d < 2^30; the state does not count in an image whose flags[1] (the segment) differs from seg (scale is not comparable
// across segments), the measurement does not count where disagree is set.
//   both count, |log2f(d_m / d_s)| <= tol:   w_d = decay w_s;  d = (w_d d_s + w_m d_m) / (w_d + w_m),  w = min(w_d + w_m, w_max)
//   both count otherwise (a NaN included):   d = d_m, w = w_m                       (the measurement replaces the state)
//   the state alone:  d = d_s, w = decay w_s;     the measurement alone:  d = d_m, w = w_m;     neither:  0, 0 (never 0 / 0)
// seg <- flags[1] by a one-thread-per-image step that runs AFTER the pixel pass, so no pixel races with it.
#pragma once
#include <string.h>

#include "pf_epipolar.h"
#include "pf_splat.h"

#define PF_RP_DMAX_MAX 65536.f

struct PfReprojArgs {
    const float* inv_depth; const float* weight; const unsigned char* mask; const float* R; const float* T;   // [B,H,W] x3, [B,9], [B,3]
    float* flow; float* d_new; unsigned char* valid;                                                        // [B,2,H,W], [B,H,W] x2
    int B, H, W; float n_min;
};
struct PfZsplatArgs {
    const float* src; const float* flow; const float* d; const float* weight; const unsigned char* valid;   // src [B,C,H,W] or null
    unsigned* front; long long* acc;                                                                        // [B,H,W], [B,C+3,H,W]
    int B, C, H, W; float b_min, ztol, w_max, dmax, vmax, fd, fn;
};
struct PfZsplatResArgs {
    long long* acc; unsigned* front; float* out; float* d_out; float* w_out; unsigned char* hole;
    int B, C, H, W; float cmin; double inv_d, ratio, w_max;
};
struct PfDepthUpdArgs {
    float* d_s; float* w_s; const float* d_m; const float* w_m; const unsigned char* disagree; const int* flags; int* seg;
    int B, H, W; float tol, decay, w_max;
};

// ---- project -----------------------------------------------------------------------------------------------------------------
PF_HD bool pf_rp_depth_ok(float d) { return d >= 0.f && d < PF_SPLAT_FAR; }                  // a NaN compares false
PF_HD bool pf_rp_identity(const float* R) {
    return R[0] == 1.f && R[4] == 1.f && R[8] == 1.f && R[1] == 0.f && R[2] == 0.f && R[3] == 0.f && R[5] == 0.f && R[6] == 0.f && R[7] == 0.f;
}
// pixel (x, y) of image b; cp, sp: pf_ego_row(y); R, T: the image's pose
PF_HD void pf_reproj_pixel(const PfReprojArgs& a, const float* R, const PfVec3& T, long b, int y, int x, float cp, float sp) {
    const long N = (long)a.H * a.W, n = (long)y * a.W + x, o = b * N + n;
    const float d = a.inv_depth[o], w = a.weight[o];
    float u = 0.f, v = 0.f, dn = 0.f;
    unsigned char ok = 0;
    if (!(a.mask && a.mask[o]) && w > 0.f && pf_rp_depth_ok(d)) {
        const PfVec3 p = pf_ego_p(x, a.W, cp, sp);
        const PfVec3 r = pf_vp_rot(R, p.x, p.y, p.z);
        PfVec3 s;
        s.x = r.x + d * T.x; s.y = r.y + d * T.y; s.z = r.z + d * T.z;
        const bool still = T.x == 0.f && T.y == 0.f && T.z == 0.f;
        const float len = still ? 1.f : pf_vp_norm(s);
        if (len >= a.n_min) {
            if (!(still && pf_rp_identity(R))) {                          // the same camera: nothing moves (the same for an image)
                float qx, qy;
                pf_vp_erp(s, a.H, a.W, qx, qy);
                const float Wf = (float)a.W;
                u = pf_pymod((qx - (float)x) + Wf * 0.5f, Wf) - Wf * 0.5f;
                v = qy - (float)y;
            }
            dn = d / len;
            ok = 1;
        }
    }
    a.flow[b * 2 * N + n] = u; a.flow[(b * 2 + 1) * N + n] = v;
    a.d_new[o] = dn;
    a.valid[o] = ok;
}

// ---- z-tested splat ------------------------------------------------------------------------------------------------------------
PF_HD unsigned pf_zs_bits(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_uint(f);
#else
    unsigned u; memcpy(&u, &f, 4); return u;
#endif
}
PF_HD float pf_zs_float(unsigned u) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(u);
#else
    float f; memcpy(&f, &u, 4); return f;
#endif
}
PF_HD void pf_zs_max(unsigned* p, unsigned v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMax(p, v);
#else
    if (v > *p) *p = v;
#endif
}
PF_HD bool pf_zs_near(float v) { return fabsf(v) < PF_SPLAT_FAR; }                         // a NaN compares false
// what a counting source pixel hands to its taps
struct PfZsPixel { float d, wn, v0, v1, v2, v3; };
// source pixel (x, y) of image b: false when it does not count; else its values and f(yy, xx, b_k) for every used tap
template <class F>
PF_HD bool pf_zsplat_taps(const PfZsplatArgs& a, long b, int y, int x, PfZsPixel& px, const F& f) {
    const int C = a.C, H = a.H, W = a.W;
    const long N = (long)H * W, n = (long)y * W + x, o = b * N + n;
    if (!a.valid[o]) return false;
    const float w = a.weight[o], d = a.d[o];
    if (!(w > 0.f) || !pf_rp_depth_ok(d)) return false;
    const float qx = (float)x + a.flow[b * 2 * N + n], qy = (float)y + a.flow[(b * 2 + 1) * N + n];
    if (!(pf_zs_near(qx) && pf_zs_near(qy))) return false;
    float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f;
    if (C > 0) {
        const float* s = a.src + b * C * N + n;
        v0 = s[0]; v1 = C > 1 ? s[N] : 0.f; v2 = C > 2 ? s[2 * N] : 0.f; v3 = C > 3 ? s[3 * N] : 0.f;
        if (!(pf_zs_near(v0) && pf_zs_near(v1) && pf_zs_near(v2) && pf_zs_near(v3))) return false;
    }
    px.d = d == 0.f ? 0.f : d;                                   // a -0 becomes +0: the bit patterns order like the values
    px.wn = (w < a.w_max ? w : a.w_max) / a.w_max;
    px.v0 = pf_splat_clamp(v0, a.vmax); px.v1 = pf_splat_clamp(v1, a.vmax); px.v2 = pf_splat_clamp(v2, a.vmax);
    px.v3 = pf_splat_clamp(v3, a.vmax);
    const float x0f = floorf(qx), y0f = floorf(qy);
    const float fx = qx - x0f, fy = qy - y0f;
    int x0 = (int)x0f % W;                                       // |x0f| < 2^30: the conversion is defined
    if (x0 < 0) x0 += W;
    const int x1 = x0 + 1 == W ? 0 : x0 + 1;
    const int y0 = (int)y0f;
    const float gx = 1.f - fx, gy = 1.f - fy;
    const float b00 = gx * gy, b01 = fx * gy, b10 = gx * fy, b11 = fx * fy;
    if (y0 >= 0 && y0 < H) {
        if (b00 >= a.b_min) f(y0, x0, b00);
        if (b01 >= a.b_min) f(y0, x1, b01);
    }
    if (y0 + 1 >= 0 && y0 + 1 < H) {
        if (b10 >= a.b_min) f(y0 + 1, x0, b10);
        if (b11 >= a.b_min) f(y0 + 1, x1, b11);
    }
    return true;
}
struct PfZsFrontTap {
    unsigned* front; int W; unsigned bits;                       // front: image b's plane
    PF_HD void operator()(int yy, int xx, float) const { pf_zs_max(front + ((long)yy * W + xx), bits); }
};
struct PfZsAccTap {
    const unsigned* front; PfSplatDirect sink; const PfZsPixel* px; int C; float ztol, dmax, fd, fn;
    PF_HD void operator()(int yy, int xx, float bk) const {
        const PfZsPixel& q = *px;
        if (!(q.d * ztol >= pf_zs_float(front[(long)yy * sink.W + xx]))) return;
        const float wb = q.wn * bk;
        if (C > 0) sink.add(0, yy, xx, pf_splat_quant(wb * q.v0, fn));
        if (C > 1) sink.add(1, yy, xx, pf_splat_quant(wb * q.v1, fn));
        if (C > 2) sink.add(2, yy, xx, pf_splat_quant(wb * q.v2, fn));
        if (C > 3) sink.add(3, yy, xx, pf_splat_quant(wb * q.v3, fn));
        sink.add(C, yy, xx, pf_splat_quant(wb * (q.d < dmax ? q.d : dmax), fn));
        sink.add(C + 1, yy, xx, pf_splat_quant(wb, fd));
        sink.add(C + 2, yy, xx, pf_splat_quant(bk, fd));
    }
};
PF_HD void pf_zsplat_front_pixel(const PfZsplatArgs& a, long b, int y, int x) {
    const long N = (long)a.H * a.W, n = (long)y * a.W + x;
    // the bits of d' are needed before the taps run: the same tests, in the same order, decide whether the pixel counts
    const float d = a.d[b * N + n];
    PfZsFrontTap f;
    f.front = a.front + b * N; f.W = a.W; f.bits = pf_zs_bits(d == 0.f ? 0.f : d);
    PfZsPixel px;
    pf_zsplat_taps(a, b, y, x, px, f);
}
PF_HD void pf_zsplat_acc_pixel(const PfZsplatArgs& a, long b, int y, int x) {
    const long N = (long)a.H * a.W;
    PfZsPixel px;
    PfZsAccTap f;
    f.front = a.front + b * N; f.px = &px; f.C = a.C; f.ztol = a.ztol; f.dmax = a.dmax; f.fd = a.fd; f.fn = a.fn;
    f.sink.N = N; f.sink.W = a.W; f.sink.acc = a.acc + b * (a.C + 3) * N;
    pf_zsplat_taps(a, b, y, x, px, f);
}

PF_HD float pf_zs_weight(long long d, long long cov, double w_max) { return (float)(w_max * ((double)d / (double)cov)); }
// target pixel n of image b
PF_HD void pf_zsplat_resolve_pixel(const PfZsplatResArgs& a, long b, long n) {
    const int C = a.C;
    const long N = (long)a.H * a.W;
    long long* p = a.acc + b * (C + 3) * N + n;
    const long long nd = p[C * N], d = p[(C + 1) * N], cov = p[(C + 2) * N];
    const bool hole = pf_splat_is_hole(d, cov, a.inv_d, a.cmin);
    for (int c = 0; c < C; ++c) {
        a.out[(b * C + c) * N + n] = hole ? 0.f : pf_splat_value(p[c * N], d, a.ratio);
        p[c * N] = 0;
    }
    p[C * N] = 0; p[(C + 1) * N] = 0; p[(C + 2) * N] = 0;
    a.front[b * N + n] = 0;
    a.d_out[b * N + n] = hole ? 0.f : pf_splat_value(nd, d, a.ratio);
    a.w_out[b * N + n] = hole ? 0.f : pf_zs_weight(d, cov, a.w_max);
    a.hole[b * N + n] = hole ? 1 : 0;
}
struct alignas(16) PfZsU4 { unsigned v[4]; };
// four consecutive target pixels n4 .. n4 + 3 (pf_zsplat_quads): the same functions on 16-byte loads and stores
PF_HD void pf_zsplat_resolve_quad(const PfZsplatResArgs& a, long b, long n4) {
    const int C = a.C;
    const long N = (long)a.H * a.W;
    long long* p = a.acc + b * (C + 3) * N + n4;
    PfSplatL2 z; z.x = 0; z.y = 0;
    PfSplatL2* pn = reinterpret_cast<PfSplatL2*>(p + C * N);
    PfSplatL2* pd = reinterpret_cast<PfSplatL2*>(p + (C + 1) * N);
    PfSplatL2* pc = reinterpret_cast<PfSplatL2*>(p + (C + 2) * N);
    const PfSplatL2 n01 = pn[0], n23 = pn[1], d01 = pd[0], d23 = pd[1], c01 = pc[0], c23 = pc[1];
    const long long nd[4] = {n01.x, n01.y, n23.x, n23.y}, d[4] = {d01.x, d01.y, d23.x, d23.y}, cv[4] = {c01.x, c01.y, c23.x, c23.y};
    PfSplatB4 hb;
    for (int k = 0; k < 4; ++k) hb.v[k] = pf_splat_is_hole(d[k], cv[k], a.inv_d, a.cmin);
    for (int c = 0; c < C; ++c) {
        PfSplatL2* ps = reinterpret_cast<PfSplatL2*>(p + c * N);
        const PfSplatL2 s01 = ps[0], s23 = ps[1];
        const long long ss[4] = {s01.x, s01.y, s23.x, s23.y};
        PfSplatF4 o;
        for (int k = 0; k < 4; ++k) o.v[k] = hb.v[k] ? 0.f : pf_splat_value(ss[k], d[k], a.ratio);
        *reinterpret_cast<PfSplatF4*>(a.out + (b * C + c) * N + n4) = o;
        ps[0] = z; ps[1] = z;
    }
    PfSplatF4 od, ow;
    for (int k = 0; k < 4; ++k) {
        od.v[k] = hb.v[k] ? 0.f : pf_splat_value(nd[k], d[k], a.ratio);
        ow.v[k] = hb.v[k] ? 0.f : pf_zs_weight(d[k], cv[k], a.w_max);
    }
    pn[0] = z; pn[1] = z; pd[0] = z; pd[1] = z; pc[0] = z; pc[1] = z;
    PfZsU4 zu; zu.v[0] = 0; zu.v[1] = 0; zu.v[2] = 0; zu.v[3] = 0;
    *reinterpret_cast<PfZsU4*>(a.front + b * N + n4) = zu;
    *reinterpret_cast<PfSplatF4*>(a.d_out + b * N + n4) = od;
    *reinterpret_cast<PfSplatF4*>(a.w_out + b * N + n4) = ow;
    *reinterpret_cast<PfSplatB4*>(a.hole + b * N + n4) = hb;
}
// the quad form needs whole quads inside a row-major image and aligned maps
static inline bool pf_zsplat_quads(const PfZsplatResArgs& a) {
    const uintptr_t bits = (uintptr_t)a.acc | (uintptr_t)a.front | (uintptr_t)a.out | (uintptr_t)a.d_out | (uintptr_t)a.w_out;
    return a.W % 4 == 0 && (bits & 15) == 0 && ((uintptr_t)a.hole & 3) == 0;
}

// ---- update ------------------------------------------------------------------------------------------------------------------
PF_HD bool pf_du_counts(float d, float w) { return w > 0.f && pf_finite(w) && pf_rp_depth_ok(d); }
// one pixel: the state (ds, ws) in place; same: the image's segment is the filter's; dis: the measurement's disagree byte
PF_HD void pf_depth_update_value(const PfDepthUpdArgs& a, bool same, float& ds, float& ws, float dm, float wm, unsigned char dis) {
    const bool cs = same && pf_du_counts(ds, ws), cm = dis == 0 && pf_du_counts(dm, wm);
    const float wsc = ws < a.w_max ? ws : a.w_max, wmc = wm < a.w_max ? wm : a.w_max;
    float d = 0.f, w = 0.f;
    if (cs && cm) {
        if (fabsf(log2f(dm / ds)) <= a.tol) {                            // 0 / 0, x / 0 and 0 / x are NaN or infinite: not within tol
            const float wd = a.decay * wsc, sum = wd + wmc;
            d = (wd * ds + wmc * dm) / sum;
            w = sum < a.w_max ? sum : a.w_max;
        } else { d = dm; w = wmc; }
    } else if (cs) { d = ds; w = a.decay * wsc; }
    else if (cm) { d = dm; w = wmc; }
    ds = d; ws = w;
}
PF_HD bool pf_du_same(const PfDepthUpdArgs& a, long b) { return a.flags[b * PF_ODO_FLAGS + 1] == a.seg[b]; }
PF_HD void pf_depth_update_pixel(const PfDepthUpdArgs& a, long b, long n) {
    const long o = b * (long)a.H * a.W + n;
    float ds = a.d_s[o], ws = a.w_s[o];
    pf_depth_update_value(a, pf_du_same(a, b), ds, ws, a.d_m[o], a.w_m[o], a.disagree ? a.disagree[o] : (unsigned char)0);
    a.d_s[o] = ds; a.w_s[o] = ws;
}
// four consecutive pixels (pf_depth_quads)
PF_HD void pf_depth_update_quad(const PfDepthUpdArgs& a, long b, long n4) {
    const long o = b * (long)a.H * a.W + n4;
    PfSplatF4 ds = *reinterpret_cast<const PfSplatF4*>(a.d_s + o), ws = *reinterpret_cast<const PfSplatF4*>(a.w_s + o);
    const PfSplatF4 dm = *reinterpret_cast<const PfSplatF4*>(a.d_m + o), wm = *reinterpret_cast<const PfSplatF4*>(a.w_m + o);
    PfSplatB4 dis; dis.v[0] = 0; dis.v[1] = 0; dis.v[2] = 0; dis.v[3] = 0;
    if (a.disagree) dis = *reinterpret_cast<const PfSplatB4*>(a.disagree + o);
    const bool same = pf_du_same(a, b);
    for (int k = 0; k < 4; ++k) pf_depth_update_value(a, same, ds.v[k], ws.v[k], dm.v[k], wm.v[k], dis.v[k]);
    *reinterpret_cast<PfSplatF4*>(a.d_s + o) = ds; *reinterpret_cast<PfSplatF4*>(a.w_s + o) = ws;
}
static inline bool pf_depth_quads(const PfDepthUpdArgs& a) {
    const uintptr_t bits = (uintptr_t)a.d_s | (uintptr_t)a.w_s | (uintptr_t)a.d_m | (uintptr_t)a.w_m;
    return ((long)a.H * a.W) % 4 == 0 && (bits & 15) == 0 && ((uintptr_t)a.disagree & 3) == 0;
}
PF_HD void pf_depth_seg_image(const PfDepthUpdArgs& a, long b) { a.seg[b] = a.flags[b * PF_ODO_FLAGS + 1]; }

// ---- argument checks shared by the device entries and their host emulation ---------------------------------------------------
static inline bool pf_rp_meet(const void* p, long np, const void* q, long nq) {
    if (!p || !q) return false;
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + (uintptr_t)nq && b < a + (uintptr_t)np;
}
// an output against every input and every output before it
static inline bool pf_rp_clash(const void* const* out, const long* outb, int nout, const void* const* in, const long* inb, int nin) {
    for (int i = 0; i < nout; ++i) {
        for (int j = 0; j < nin; ++j) if (pf_rp_meet(out[i], outb[i], in[j], inb[j])) return true;
        for (int j = 0; j < i; ++j) if (pf_rp_meet(out[i], outb[i], out[j], outb[j])) return true;
    }
    return false;
}
static inline bool pf_rp_pos(float v) { return v > 0.f && pf_finite(v); }
// the shape limits of pf_splat_geometry, with C = 0 allowed
static inline int pf_rp_geometry(int B, int C, int H, int W) {
    if (C < 0 || C > 4) return PF_ERR_BAD_ARG;
    if (B < 1 || H < 1 || W < 1 || (long)H * W >= (1L << 30) || B > PF_SPLAT_MAX_GRID) return PF_ERR_BAD_SHAPE;
    return PF_OK;
}
static inline bool pf_rp_misaligned(const void* p, int mask) { return ((uintptr_t)p & (uintptr_t)mask) != 0; }

static inline int pf_reproj_project_check(const float* inv_depth, const float* weight, const unsigned char* mask, const float* R,
                                          const float* T, float* flow, float* d_new, unsigned char* valid, int B, int H, int W,
                                          float n_min, PfReprojArgs& a) {
    if (!inv_depth || !weight || !R || !T || !flow || !d_new || !valid) return PF_ERR_BAD_ARG;
    if (pf_rp_misaligned(inv_depth, 3) || pf_rp_misaligned(weight, 3) || pf_rp_misaligned(R, 3) || pf_rp_misaligned(T, 3)
        || pf_rp_misaligned(flow, 3) || pf_rp_misaligned(d_new, 3)) return PF_ERR_BAD_ARG;
    if (!pf_rp_pos(n_min)) return PF_ERR_BAD_ARG;
    const int rc = pf_rp_geometry(B, 0, H, W);
    if (rc != PF_OK) return rc;
    const long N = (long)B * H * W;
    const void* in[5] = {inv_depth, weight, mask, R, T};
    const long inb[5] = {N * 4, N * 4, N, (long)B * 36, (long)B * 12};
    const void* out[3] = {flow, d_new, valid};
    const long outb[3] = {N * 8, N * 4, N};
    if (pf_rp_clash(out, outb, 3, in, inb, 5)) return PF_ERR_BAD_ARG;
    a.inv_depth = inv_depth; a.weight = weight; a.mask = mask; a.R = R; a.T = T; a.flow = flow; a.d_new = d_new; a.valid = valid;
    a.B = B; a.H = H; a.W = W; a.n_min = n_min;
    return PF_OK;
}
static inline long pf_zsplat_acc_bytes(int B, int C, int H, int W) {
    const int rc = pf_rp_geometry(B, C, H, W);
    return rc != PF_OK ? rc : (long)B * (C + 3) * H * W * 8;
}
// front and accumulate: the inputs, the two buffers and the parameters (front's call passes acc = null and the defaults it does
// not read)
static inline int pf_zsplat_check(const float* src, const float* flow, const float* d, const float* weight, const unsigned char* valid,
                                  void* front, void* acc, bool need_acc, int B, int C, int H, int W, float b_min, float tol_log2,
                                  float w_max, float dmax, float vmax, PfZsplatArgs& a) {
    if (!flow || !d || !weight || !valid || !front || (need_acc && !acc)) return PF_ERR_BAD_ARG;
    const int rc = pf_rp_geometry(B, C, H, W);
    if (rc != PF_OK) return rc;
    if ((C > 0) != (src != nullptr)) return PF_ERR_BAD_ARG;
    if (pf_rp_misaligned(src, 3) || pf_rp_misaligned(flow, 3) || pf_rp_misaligned(d, 3) || pf_rp_misaligned(weight, 3)
        || pf_rp_misaligned(front, 3) || pf_rp_misaligned(acc, 7)) return PF_ERR_BAD_ARG;
    if (!(b_min >= 0.f && b_min <= 1.f) || !(tol_log2 >= 0.f && tol_log2 <= 64.f) || !pf_rp_pos(w_max)) return PF_ERR_BAD_ARG;
    if (!(dmax >= 1.f && dmax <= PF_RP_DMAX_MAX) || !(vmax >= 1.f && vmax <= PF_SPLAT_VMAX_MAX)) return PF_ERR_BAD_ARG;
    const long N = (long)B * H * W;
    const void* in[5] = {src, flow, d, weight, valid};
    const long inb[5] = {N * 4 * C, N * 8, N * 4, N * 4, N};
    const void* out[2] = {front, acc};
    const long outb[2] = {N * 4, N * 8 * (C + 3)};
    if (pf_rp_clash(out, outb, 2, in, inb, 5)) return PF_ERR_BAD_ARG;
    const PfSplatScales s = pf_splat_scales(1, H, W, dmax > vmax ? dmax : vmax);
    a.src = src; a.flow = flow; a.d = d; a.weight = weight; a.valid = valid; a.front = static_cast<unsigned*>(front);
    a.acc = static_cast<long long*>(acc); a.B = B; a.C = C; a.H = H; a.W = W; a.b_min = b_min; a.ztol = exp2f(tol_log2);
    a.w_max = w_max; a.dmax = dmax; a.vmax = vmax; a.fd = s.fd; a.fn = s.fn;
    return PF_OK;
}
static inline int pf_zsplat_resolve_check(void* acc, void* front, float* out, float* d_out, float* w_out, unsigned char* hole, int B,
                                          int C, int H, int W, float cmin, float w_max, float dmax, float vmax, PfZsplatResArgs& a) {
    if (!acc || !front || !d_out || !w_out || !hole) return PF_ERR_BAD_ARG;
    const int rc = pf_rp_geometry(B, C, H, W);
    if (rc != PF_OK) return rc;
    if ((C > 0) != (out != nullptr)) return PF_ERR_BAD_ARG;
    if (pf_rp_misaligned(acc, 7) || pf_rp_misaligned(front, 3) || pf_rp_misaligned(out, 3) || pf_rp_misaligned(d_out, 3)
        || pf_rp_misaligned(w_out, 3)) return PF_ERR_BAD_ARG;
    if (!pf_rp_pos(cmin) || !pf_rp_pos(w_max)) return PF_ERR_BAD_ARG;
    if (!(dmax >= 1.f && dmax <= PF_RP_DMAX_MAX) || !(vmax >= 1.f && vmax <= PF_SPLAT_VMAX_MAX)) return PF_ERR_BAD_ARG;
    const long N = (long)B * H * W;
    const void* bufs[6] = {acc, front, out, d_out, w_out, hole};
    const long bufb[6] = {N * 8 * (C + 3), N * 4, N * 4 * C, N * 4, N * 4, N};
    if (pf_rp_clash(bufs, bufb, 6, nullptr, nullptr, 0)) return PF_ERR_BAD_ARG;
    const PfSplatScales s = pf_splat_scales(1, H, W, dmax > vmax ? dmax : vmax);
    a.acc = static_cast<long long*>(acc); a.front = static_cast<unsigned*>(front); a.out = out; a.d_out = d_out; a.w_out = w_out;
    a.hole = hole; a.B = B; a.C = C; a.H = H; a.W = W; a.cmin = cmin; a.inv_d = s.inv_d; a.ratio = s.ratio; a.w_max = (double)w_max;
    return PF_OK;
}
static inline int pf_depth_update_check(float* d_s, float* w_s, const float* d_m, const float* w_m, const unsigned char* disagree,
                                        const int* flags, int* seg, int B, int H, int W, float tol_log2, float decay, float w_max,
                                        PfDepthUpdArgs& a) {
    if (!d_s || !w_s || !d_m || !w_m || !flags || !seg) return PF_ERR_BAD_ARG;
    if (pf_rp_misaligned(d_s, 3) || pf_rp_misaligned(w_s, 3) || pf_rp_misaligned(d_m, 3) || pf_rp_misaligned(w_m, 3)
        || pf_rp_misaligned(flags, 3) || pf_rp_misaligned(seg, 3)) return PF_ERR_BAD_ARG;
    if (!pf_rp_pos(tol_log2) || !(decay > 0.f && decay <= 1.f) || !pf_rp_pos(w_max)) return PF_ERR_BAD_ARG;
    const int rc = pf_rp_geometry(B, 0, H, W);
    if (rc != PF_OK) return rc;
    const long N = (long)B * H * W;
    const void* in[4] = {d_m, w_m, disagree, flags};
    const long inb[4] = {N * 4, N * 4, N, (long)B * PF_ODO_FLAGS * 4};
    const void* out[3] = {d_s, w_s, seg};
    const long outb[3] = {N * 4, N * 4, (long)B * 4};
    if (pf_rp_clash(out, outb, 3, in, inb, 4)) return PF_ERR_BAD_ARG;
    a.d_s = d_s; a.w_s = w_s; a.d_m = d_m; a.w_m = w_m; a.disagree = disagree; a.flags = flags; a.seg = seg;
    a.B = B; a.H = H; a.W = W; a.tol = tol_log2; a.decay = decay; a.w_max = w_max;
    return PF_OK;
}
