// Forward softmax splatting with order-independent sums (include/priorflow_hip.h: pf_splat_accumulate,
// pf_splat_resolve).  The statement, once, for the device kernels (pf_splat.hip), the host emulation (tests/emu/pf_emu_splat.cpp)
// and the C checks.
//
// A call has 1..PF_SPLAT_MAX jobs on one grid [B,*,H,W]: a source map src (C = 1..4 planes), a flow, an optional metric
// (Cm = 1: m = |metric|; Cm = 2: m = sqrt(m0^2 + m1^2), all in fp32), an optional byte mask (non-zero: skip), tau and beta.
// Source pixel s = (x, y) of job j, every step a rounded fp32 operation (the units are built without contraction):
//   q  = (x + tau u, y + tau v)
//   w  = beta expf(-min(alpha m, zmax)), or beta when there is no metric or alpha == 0 (no expf is evaluated then)
//   the pixel is skipped when it is masked, or when q, m or one of its C values is not finite; a coordinate of q at or beyond
//   PF_SPLAT_FAR = 2^30 pixels counts as not finite (the integer conversion below happens after this test, never before)
//   x0 = floor(qx), y0 = floor(qy), fx = qx - x0, fy = qy - y0; columns x0, x0 + 1 wrapped with the Python modulo; rows y0,
//   y0 + 1, a row outside [0, H - 1] DROPPED, not clamped; b_k = {1 - fx, fx} x {1 - fy, fy}; a tap with b_k = 0 adds nothing
//   N_c[p] += (w b_k) clamp(src_c, +-vmax),   D[p] += w b_k,   cov[p] += beta b_k
// Resolve, per target p: hole = cov < cmin (or D <= 0: nothing to divide by); out_c = N_c / D, a hole takes the fill
// (1 - t) fill0[p] + t fill1[p], or 0 without fill maps.
//
// N, D and cov are 64-bit integers: a contribution is llrintf(value * 2^S), value the fp32 product above.  Integer adds commute,
// so a result does not depend on the order in which the adds arrive.  pf_splat_scales gives S for both sides from
// (njobs, H, W, vmax) alone:
//   S_D = S_cov = 62 - ceil(log2(njobs H W)),   S_N = S_D - ceil(log2(vmax)).
// Per image a job's pixel spreads sum b_k = 1 with w <= beta <= 1, so |D|, |cov| <= njobs H W and |N_c| <= njobs H W vmax before
// scaling: every sum stays below 2^62 in magnitude whatever the flow does; the 4 njobs H W roundings of at most 1/2 each do not
// reach the remaining bit.
#pragma once
#include "pf_common.h"
#include "pf_elem.h"                          // pf_finite, pf_pick4
#include "../../include/priorflow_hip.h"      // PF_SPLAT_MAX, pf_splat_job; checks the definitions against their declarations

#define PF_SPLAT_FAR 1073741824.f             // 2^30
#define PF_SPLAT_VMAX_MAX 65536.f
#define PF_SPLAT_MAX_GRID 65535

struct PfSplatJob {
    const float* src; const float* flow;      // [B,C,H,W], [B,2,H,W]
    const float* metric;                      // [B,cm,H,W] or null
    const unsigned char* mask;                // [B,H,W] or null
    int cm; float tau, beta;
};
struct PfSplatAccArgs { PfSplatJob job[PF_SPLAT_MAX]; long long* acc; int njobs, B, C, H, W; float alpha, zmax, vmax, fd, fn; };
struct PfSplatResArgs {
    long long* acc; float* out; unsigned char* hole; const float* fill0; const float* fill1;
    float fill_t, cmin; int B, C, H, W; double inv_d, ratio;
};

// the scales of one call, for the accumulate side (fd = 2^S_D, fn = 2^S_N) and the resolve side (inv_d = 2^-S_D,
// ratio = 2^(S_D - S_N)): ONE function, so the two sides cannot disagree
struct PfSplatScales { int sd, sn; float fd, fn; double inv_d, ratio; };
static inline PfSplatScales pf_splat_scales(int njobs, int H, int W, float vmax) {
    const long n = (long)njobs * H * W;
    int lg = 0, lv = 0;
    while ((1L << lg) < n) ++lg;
    while (ldexpf(1.f, lv) < vmax) ++lv;
    PfSplatScales s;
    s.sd = 62 - lg; s.sn = s.sd - lv;
    s.fd = ldexpf(1.f, s.sd); s.fn = ldexpf(1.f, s.sn);
    s.inv_d = ldexp(1.0, -s.sd); s.ratio = ldexp(1.0, lv);
    return s;
}

// job j, field by field from values loaded with constant indices (pf_compose_pick: an argument indexed by a run-time value
// would be copied to scratch memory)
#define PF_SPLAT_FIELD(m) pf_pick4(j, a.job[0].m, a.job[1].m, a.job[2].m, a.job[3].m)
PF_HD PfSplatJob pf_splat_pick(const PfSplatAccArgs& a, int j) {
    PfSplatJob q;
    q.src = PF_SPLAT_FIELD(src); q.flow = PF_SPLAT_FIELD(flow); q.metric = PF_SPLAT_FIELD(metric); q.mask = PF_SPLAT_FIELD(mask);
    q.cm = PF_SPLAT_FIELD(cm); q.tau = PF_SPLAT_FIELD(tau); q.beta = PF_SPLAT_FIELD(beta);
    return q;
}
#undef PF_SPLAT_FIELD

// one add into a sum: on the device a 64-bit integer atomic whose result nobody reads, on the host a plain add
PF_HD void pf_splat_add(long long* p, long long v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
#else
    *p += v;
#endif
}
PF_HD long long pf_splat_quant(float value, float scale) { return llrintf(value * scale); }

// where a contribution goes: plane 0..C-1 = N_c, C = D, C + 1 = cov of image b, target (yy, xx) inside the map.  PfSplatDirect adds
// straight into the sums; the device's windowed launch (pf_splat.hip) puts another sink in front of it
struct PfSplatDirect {
    long long* acc; long N; int W;                               // acc: image b's planes
    PF_HD void add(int plane, int yy, int xx, long long v) const { pf_splat_add(acc + plane * N + ((long)yy * W + xx), v); }
};
// one tap (row yy, column xx) of a source pixel: bk = its bilinear weight, w the pixel's importance, v its clamped values
template <class Sink>
PF_HD void pf_splat_tap(const Sink& s, int C, int H, int yy, int xx, float bk, float w, float beta, float v0, float v1, float v2,
                        float v3, float fd, float fn) {
    if (yy < 0 || yy >= H || !(bk > 0.f)) return;               // past a pole: dropped; xx is inside [0, W) by construction
    const float wb = w * bk;
    s.add(0, yy, xx, pf_splat_quant(wb * v0, fn));
    if (C > 1) s.add(1, yy, xx, pf_splat_quant(wb * v1, fn));
    if (C > 2) s.add(2, yy, xx, pf_splat_quant(wb * v2, fn));
    if (C > 3) s.add(3, yy, xx, pf_splat_quant(wb * v3, fn));
    s.add(C, yy, xx, pf_splat_quant(wb, fd));
    s.add(C + 1, yy, xx, pf_splat_quant(beta * bk, fd));
}
PF_HD float pf_splat_clamp(float v, float vmax) { return v < -vmax ? -vmax : (v > vmax ? vmax : v); }

// source pixel (x, y) of image b of job q into the sink
template <class Sink>
PF_HD void pf_splat_pixel_to(const PfSplatJob& q, const PfSplatAccArgs& a, long b, int y, int x, const Sink& sink) {
    const int C = a.C, H = a.H, W = a.W;
    const long N = (long)H * W, n = (long)y * W + x;
    if (q.mask && q.mask[b * N + n]) return;
    const float* fl = q.flow + b * 2 * N;
    const float qx = (float)x + q.tau * fl[n], qy = (float)y + q.tau * fl[N + n];
    if (!(fabsf(qx) < PF_SPLAT_FAR && fabsf(qy) < PF_SPLAT_FAR)) return;       // a NaN compares false
    float w = q.beta;
    if (q.metric) {
        const float* mp = q.metric + b * q.cm * N;
        const float m0 = mp[n];
        const float m = q.cm == 2 ? sqrtf(m0 * m0 + mp[N + n] * mp[N + n]) : fabsf(m0);
        if (!pf_finite(m)) return;
        if (a.alpha > 0.f) {
            float z = a.alpha * m;
            z = z < a.zmax ? z : a.zmax;
            w = q.beta * expf(-z);
        }
    }
    const float* s = q.src + b * C * N + n;
    float v0 = s[0], v1 = C > 1 ? s[N] : 0.f, v2 = C > 2 ? s[2 * N] : 0.f, v3 = C > 3 ? s[3 * N] : 0.f;
    if (!(pf_finite(v0) && pf_finite(v1) && pf_finite(v2) && pf_finite(v3))) return;
    v0 = pf_splat_clamp(v0, a.vmax); v1 = pf_splat_clamp(v1, a.vmax); v2 = pf_splat_clamp(v2, a.vmax); v3 = pf_splat_clamp(v3, a.vmax);
    const float x0f = floorf(qx), y0f = floorf(qy);
    const float fx = qx - x0f, fy = qy - y0f;
    int x0 = (int)x0f % W;                                       // |x0f| < 2^30: the conversion is defined
    if (x0 < 0) x0 += W;
    const int x1 = x0 + 1 == W ? 0 : x0 + 1;
    const int y0 = (int)y0f;
    const float gx = 1.f - fx, gy = 1.f - fy;
    pf_splat_tap(sink, C, H, y0, x0, gx * gy, w, q.beta, v0, v1, v2, v3, a.fd, a.fn);
    pf_splat_tap(sink, C, H, y0, x1, fx * gy, w, q.beta, v0, v1, v2, v3, a.fd, a.fn);
    pf_splat_tap(sink, C, H, y0 + 1, x0, gx * fy, w, q.beta, v0, v1, v2, v3, a.fd, a.fn);
    pf_splat_tap(sink, C, H, y0 + 1, x1, fx * fy, w, q.beta, v0, v1, v2, v3, a.fd, a.fn);
}
PF_HD PfSplatDirect pf_splat_direct(const PfSplatAccArgs& a, long b) {
    PfSplatDirect d;
    d.N = (long)a.H * a.W; d.W = a.W; d.acc = a.acc + b * (a.C + 2) * d.N;
    return d;
}
// ... straight into the sums [B][C+2][H][W]
PF_HD void pf_splat_pixel(const PfSplatJob& q, const PfSplatAccArgs& a, long b, int y, int x) {
    pf_splat_pixel_to(q, a, b, y, x, pf_splat_direct(a, b));
}

// ---- resolve ---------------------------------------------------------------------------------------------------------------------
PF_HD bool pf_splat_is_hole(long long d, long long cov, double inv_d, float cmin) {
    return !((double)cov * inv_d >= (double)cmin) || d <= 0;
}
PF_HD float pf_splat_value(long long n, long long d, double ratio) { return (float)(((double)n / (double)d) * ratio); }
PF_HD float pf_splat_fill(const float* fill0, const float* fill1, long i, float t) {
    return fill0 ? (1.f - t) * fill0[i] + t * fill1[i] : 0.f;
}
// target pixel n of image b: reads the C + 2 sums, writes C floats and the hole byte, and zeros over the sums it read
PF_HD void pf_splat_resolve_pixel(const PfSplatResArgs& a, long b, long n) {
    const int C = a.C;
    const long N = (long)a.H * a.W;
    long long* p = a.acc + b * (C + 2) * N + n;
    const long long d = p[C * N], cov = p[(C + 1) * N];
    const bool hole = pf_splat_is_hole(d, cov, a.inv_d, a.cmin);
    for (int c = 0; c < C; ++c) {
        const long i = (b * C + c) * N + n;
        a.out[i] = hole ? pf_splat_fill(a.fill0, a.fill1, i, a.fill_t) : pf_splat_value(p[c * N], d, a.ratio);
        p[c * N] = 0;
    }
    p[C * N] = 0; p[(C + 1) * N] = 0;
    a.hole[b * N + n] = hole ? 1 : 0;
}
// four consecutive target pixels n4 .. n4 + 3 (n4 % 4 == 0, every map 16-byte aligned, N % 4 == 0): the same functions on 16-byte
// loads and stores
struct alignas(16) PfSplatL2 { long long x, y; };
struct alignas(16) PfSplatF4 { float v[4]; };
struct alignas(4) PfSplatB4 { unsigned char v[4]; };
PF_HD void pf_splat_resolve_quad(const PfSplatResArgs& a, long b, long n4) {
    const int C = a.C;
    const long N = (long)a.H * a.W;
    long long* p = a.acc + b * (C + 2) * N + n4;
    PfSplatL2 z; z.x = 0; z.y = 0;
    PfSplatL2* pd = reinterpret_cast<PfSplatL2*>(p + C * N);
    PfSplatL2* pc = reinterpret_cast<PfSplatL2*>(p + (C + 1) * N);
    const PfSplatL2 d01 = pd[0], d23 = pd[1], c01 = pc[0], c23 = pc[1];
    const long long d[4] = {d01.x, d01.y, d23.x, d23.y};
    PfSplatB4 hb;
    hb.v[0] = pf_splat_is_hole(d[0], c01.x, a.inv_d, a.cmin); hb.v[1] = pf_splat_is_hole(d[1], c01.y, a.inv_d, a.cmin);
    hb.v[2] = pf_splat_is_hole(d[2], c23.x, a.inv_d, a.cmin); hb.v[3] = pf_splat_is_hole(d[3], c23.y, a.inv_d, a.cmin);
    for (int c = 0; c < C; ++c) {
        PfSplatL2* pn = reinterpret_cast<PfSplatL2*>(p + c * N);
        const PfSplatL2 n01 = pn[0], n23 = pn[1];
        const long long nn[4] = {n01.x, n01.y, n23.x, n23.y};
        const long i = (b * C + c) * N + n4;
        PfSplatF4 o;
        for (int k = 0; k < 4; ++k)
            o.v[k] = hb.v[k] ? pf_splat_fill(a.fill0, a.fill1, i + k, a.fill_t) : pf_splat_value(nn[k], d[k], a.ratio);
        *reinterpret_cast<PfSplatF4*>(a.out + i) = o;
        pn[0] = z; pn[1] = z;
    }
    pd[0] = z; pd[1] = z; pc[0] = z; pc[1] = z;
    *reinterpret_cast<PfSplatB4*>(a.hole + b * N + n4) = hb;
}
// the quad form needs whole quads inside a row-major image and aligned maps
static inline bool pf_splat_quads(const PfSplatResArgs& a) {
    const uintptr_t bits = (uintptr_t)a.acc | (uintptr_t)a.out | (uintptr_t)a.fill0 | (uintptr_t)a.fill1;
    return a.W % 4 == 0 && (bits & 15) == 0 && ((uintptr_t)a.hole & 3) == 0;
}

// ---- argument checks shared by the device entries and their host emulation ---------------------------------------------------
static inline int pf_splat_geometry(int njobs, int B, int C, int H, int W, float vmax) {
    if (njobs < 1 || njobs > PF_SPLAT_MAX || C < 1 || C > 4) return PF_ERR_BAD_ARG;
    if (!(vmax >= 1.f && vmax <= PF_SPLAT_VMAX_MAX)) return PF_ERR_BAD_ARG;
    if (B < 1 || H < 1 || W < 1 || (long)H * W >= (1L << 30) || B > PF_SPLAT_MAX_GRID) return PF_ERR_BAD_SHAPE;
    return PF_OK;
}
static inline int pf_splat_accumulate_check(const pf_splat_job* jobs, int njobs, void* acc, int B, int C, int H, int W, float alpha,
                                            float zmax, float vmax, PfSplatAccArgs& a) {
    if (!jobs || !acc || ((uintptr_t)acc & 7)) return PF_ERR_BAD_ARG;
    int rc = pf_splat_geometry(njobs, B, C, H, W, vmax);
    if (rc != PF_OK) return rc;
    if (!(alpha >= 0.f && pf_finite(alpha)) || !(zmax >= 0.f && pf_finite(zmax))) return PF_ERR_BAD_ARG;
    for (int i = 0; i < PF_SPLAT_MAX; ++i) {
        const pf_splat_job& j = jobs[i < njobs ? i : 0];           // the unused rows repeat job 0 and are never run
        if (!j.src || !j.flow || (const void*)j.src == acc || (const void*)j.flow == acc) return PF_ERR_BAD_ARG;
        if (j.metric && j.cm != 1 && j.cm != 2) return PF_ERR_BAD_ARG;
        if (!pf_finite(j.tau) || !(j.beta > 0.f && j.beta <= 1.f)) return PF_ERR_BAD_ARG;
        PfSplatJob& q = a.job[i];
        q.src = j.src; q.flow = j.flow; q.metric = j.metric; q.mask = j.mask; q.cm = j.metric ? j.cm : 1; q.tau = j.tau; q.beta = j.beta;
    }
    const PfSplatScales s = pf_splat_scales(njobs, H, W, vmax);
    a.acc = static_cast<long long*>(acc); a.njobs = njobs; a.B = B; a.C = C; a.H = H; a.W = W;
    a.alpha = alpha; a.zmax = zmax; a.vmax = vmax; a.fd = s.fd; a.fn = s.fn;
    return PF_OK;
}
static inline int pf_splat_resolve_check(void* acc, float* out, unsigned char* hole, const float* fill0, const float* fill1,
                                         float fill_t, float cmin, int njobs, int B, int C, int H, int W, float vmax,
                                         PfSplatResArgs& a) {
    if (!acc || !out || !hole || ((uintptr_t)acc & 7) || (void*)out == acc || (void*)hole == acc || (void*)hole == (void*)out)
        return PF_ERR_BAD_ARG;
    if ((fill0 == nullptr) != (fill1 == nullptr)) return PF_ERR_BAD_ARG;
    if (fill0 && (out == fill0 || out == fill1 || !(fill_t >= 0.f && fill_t <= 1.f))) return PF_ERR_BAD_ARG;   // out aliasing a source
    if (!(cmin > 0.f && pf_finite(cmin))) return PF_ERR_BAD_ARG;
    const int rc = pf_splat_geometry(njobs, B, C, H, W, vmax);
    if (rc != PF_OK) return rc;
    const PfSplatScales s = pf_splat_scales(njobs, H, W, vmax);
    a.acc = static_cast<long long*>(acc); a.out = out; a.hole = hole; a.fill0 = fill0; a.fill1 = fill1;
    a.fill_t = fill0 ? fill_t : 0.f; a.cmin = cmin; a.B = B; a.C = C; a.H = H; a.W = W; a.inv_d = s.inv_d; a.ratio = s.ratio;
    return PF_OK;
}
static inline long pf_splat_bytes(int B, int C, int H, int W) {
    if (B < 1 || C < 1 || C > 4 || H < 1 || W < 1 || (long)H * W >= (1L << 30) || B > PF_SPLAT_MAX_GRID) return PF_ERR_BAD_SHAPE;
    return (long)B * (C + 2) * H * W * 8;
}
