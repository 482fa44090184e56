// Camera rotation from a full-sphere flow field, and what follows from it (include/priorflow_hip.h:
// pf_ego_accumulate, pf_ego_solve, pf_ego_track, pf_erp_rotate, pf_ego_derotate).  The statement, once, for the device kernels
// (pf_egomotion.hip), the host emulation (tests/emu/pf_emu_egomotion.cpp) and the C checks.  The geometry is pf_viewport.h's
// (pf_vp_sphere = s, pf_vp_erp = erp); nothing of it is restated here.
//
// Pixel (x, y) of image b of an H x W ERP flow (u, v), every step a rounded fp32 operation (the units are built without contraction):
//   p = s(x, y),   q = s(x + (u mod W), clamp(y + v, -1/2, H - 1/2))        (flow2endpoint's rule, as pf_vp_flow_pixel)
//   u mod W is the Python modulo, exact in fp32: the bearing is periodic, so u and u +- W give the same q up to the rounding of the
//   caller's own u +- W, and a zero flow gives q == p bit for bit.
//   The pixel is LEFT OUT when its mask byte is non-zero or when |u| or |v| is not below PF_EGO_FAR = 2^30 pixels (a NaN compares
//   false); that test comes before any other use of u or v.
// The rotation sought has q ~ R p.  Pass k of an estimate weighs the pixel with w = cos phi(y) g_k: cos phi is its solid angle,
// g_0 = 1, and for k >= 1 g_k = 1 / (1 + r^2 / c^2)^2 (Geman-McClure) of the chord r = |q - R_{k-1} p|, c = scale_px 2 pi / W.
// r^2 is clamped to 4, NaN included, so whatever the matrix in memory holds every weight lies in [0, 1].
//
// Twelve sums per image: S_ab = sum w p_a q_b (a * 3 + b), 9: sum w, 10: sum w r^2, 11: the number of pixels used.  They are 64-bit
// integers, a contribution llrintf(value * 2^S) of the fp32 value, so the adds commute and the result is the same bits on every
// run and for every grid.  pf_ego_scales gives S for both sides from (H, W) alone:
//   S = 62 - ceil(log2(H W)) for S_ab and sum w (|w p_a q_b| <= 1, w <= 1),  S - 2 for sum w r^2 (r^2 <= 4).
// Worst case: every one of the H W pixels at the maximum adds 2^S <= 2^62 / (H W), a sum of at most 2^62; the H W roundings of
// at most 1/2 each do not reach the remaining bit.
//
// Solve, per image, in fp64: Horn's symmetric 4 x 4 matrix N of S, its eigenvectors by PF_EGO_SWEEPS cyclic Jacobi sweeps, the
// unit quaternion (a, b, c, d) of the largest eigenvalue with a >= 0, R its matrix.  stats = {sum w, sqrt(sum w r^2 / sum w),
// used / (H W), gap = (lambda_1 - lambda_2) / sum w, valid}; valid = 0 when sum w = 0 or gap < gap_min, and then R is init (the
// identity without one).  The solve writes zeros over the sums it read.
#pragma once
#include "pf_viewport.h"

#define PF_EGO_FAR 1073741824.f               // 2^30
#define PF_EGO_SWEEPS 8
#define PF_EGO_MAX_GRID 65535
static_assert(PF_EGO_SUMS == 12 && PF_EGO_STATS == 5 && PF_EGO_STATE == 8, "the sizes of pf_egomotion.h and of the public header");

struct PfEgoAccArgs {
    const float* flow; const unsigned char* mask; const float* R;        // [B,2,H,W], [B,H,W] or null, [B,9]
    long long* sums;                                                      // [B,12]
    int B, H, W, weighted; float inv_c2, f, fr;
};
struct PfEgoSolveArgs { long long* sums; const float* init; float* R; float* stats; int B, H, W; float gap_min; double inv, inv_r; };
struct PfEgoTrackArgs { const float* R; double* state; float* orient; float* corr; int B; double t; };
struct PfErpRotArgs { const void* in; void* out; const float* R; int B, C, H, W, form; };
struct PfEgoDerotArgs { const float* flow; const unsigned char* mask; const float* R; float* out; unsigned char* valid; int B, H, W; };

// the scales of one geometry, for the accumulating side (f = 2^S, fr = 2^(S-2)) and the solving side (their inverses): ONE
// function, so the two sides cannot disagree
struct PfEgoScales { int s, sr; float f, fr; double inv, inv_r; };
static inline PfEgoScales pf_ego_scales(int H, int W) {
    const long n = (long)H * W;
    int lg = 0;
    while ((1L << lg) < n) ++lg;
    PfEgoScales s;
    s.s = 62 - lg; s.sr = s.s - 2;
    s.f = ldexpf(1.f, s.s); s.fr = ldexpf(1.f, s.sr);
    s.inv = ldexp(1.0, -s.s); s.inv_r = ldexp(1.0, -s.sr);
    return s;
}

// ---- the two bearings of a pixel ---------------------------------------------------------------------------------------------
PF_HD bool pf_ego_left_out(float u, float v, unsigned char m) { return m != 0 || !(fabsf(u) < PF_EGO_FAR && fabsf(v) < PF_EGO_FAR); }
// cos phi(y), sin phi(y): the same for a whole row
PF_HD void pf_ego_row(int y, int H, float& cp, float& sp) { const float p = pf_vp_phi((float)y, H); cp = cosf(p); sp = sinf(p); }
// p = s(x, y) from the row's values: pf_vp_sphere's expressions on the same bits
PF_HD PfVec3 pf_ego_p(int x, int W, float cp, float sp) { const float t = pf_vp_theta((float)x, W); return pf_vp_dir(cosf(t), sinf(t), cp, sp); }
PF_HD PfVec3 pf_ego_q(int x, int y, float u, float v, int H, int W) {
    float ey = (float)y + v;
    ey = ey < -0.5f ? -0.5f : (ey > (float)H - 0.5f ? (float)H - 0.5f : ey);
    return pf_vp_sphere((float)x + pf_pymod(u, (float)W), ey, H, W);
}
PF_HD float pf_ego_chord2(const float* R, const PfVec3& p, const PfVec3& q) {
    const PfVec3 rp = pf_vp_rot(R, p.x, p.y, p.z);
    const float dx = q.x - rp.x, dy = q.y - rp.y, dz = q.z - rp.z;
    const float r2 = (dx * dx + dy * dy) + dz * dz;
    return r2 <= 4.f ? r2 : 4.f;                                          // a NaN takes the clamp
}
PF_HD long long pf_ego_quant(float value, float scale) { return llrintf(value * scale); }

// pixel (x, y) with flow (u, v) and mask byte m into the twelve partial sums s; cp, sp: pf_ego_row(y); R: the image's R_{k-1}
PF_HD void pf_ego_pixel(const PfEgoAccArgs& a, const float* R, float cp, float sp, int y, int x, float u, float v, unsigned char m,
                        long long* s) {
    if (pf_ego_left_out(u, v, m)) return;
    const PfVec3 p = pf_ego_p(x, a.W, cp, sp), q = pf_ego_q(x, y, u, v, a.H, a.W);
    const float r2 = pf_ego_chord2(R, p, q);
    float w = cp;
    if (a.weighted) {
        const float t = 1.f + r2 * a.inv_c2;
        w = cp * (1.f / (t * t));
    }
    const float wx = w * p.x, wy = w * p.y, wz = w * p.z;
    s[0] += pf_ego_quant(wx * q.x, a.f); s[1] += pf_ego_quant(wx * q.y, a.f); s[2] += pf_ego_quant(wx * q.z, a.f);
    s[3] += pf_ego_quant(wy * q.x, a.f); s[4] += pf_ego_quant(wy * q.y, a.f); s[5] += pf_ego_quant(wy * q.z, a.f);
    s[6] += pf_ego_quant(wz * q.x, a.f); s[7] += pf_ego_quant(wz * q.y, a.f); s[8] += pf_ego_quant(wz * q.z, a.f);
    s[9] += pf_ego_quant(w, a.f);
    s[10] += pf_ego_quant(w * r2, a.fr);
    s[11] += 1;
}

// ---- quaternions (a, b, c, d) = (scalar, vector), fp64 -----------------------------------------------------------------------
struct PfQuat { double a, b, c, d; };
PF_HD PfQuat pf_quat_unit(PfQuat q) {
    const double n = sqrt((q.a * q.a + q.b * q.b) + (q.c * q.c + q.d * q.d));
    if (!(n > 0.0)) { q.a = 1.0; q.b = 0.0; q.c = 0.0; q.d = 0.0; return q; }     // nothing to normalise (NaN included): identity
    q.a /= n; q.b /= n; q.c /= n; q.d /= n;
    return q;
}
// the unit quaternion with a non-negative scalar part: of the two that name a rotation the one every holder of a state agrees on
PF_HD PfQuat pf_quat_canon(PfQuat q) {
    q = pf_quat_unit(q);
    if (q.a < 0.0) { q.a = -q.a; q.b = -q.b; q.c = -q.c; q.d = -q.d; }
    return q;
}
PF_HD PfQuat pf_quat_mul(const PfQuat& x, const PfQuat& y) {            // the rotation of y, then that of x
    PfQuat o;
    o.a = x.a * y.a - x.b * y.b - x.c * y.c - x.d * y.d;
    o.b = x.a * y.b + x.b * y.a + x.c * y.d - x.d * y.c;
    o.c = x.a * y.c - x.b * y.d + x.c * y.a + x.d * y.b;
    o.d = x.a * y.d + x.b * y.c - x.c * y.b + x.d * y.a;
    return o;
}
PF_HD PfQuat pf_quat_conj(const PfQuat& q) { PfQuat o; o.a = q.a; o.b = -q.b; o.c = -q.c; o.d = -q.d; return o; }
// the matrix of a unit quaternion, nine fp32 values row-major
PF_HD void pf_quat_matrix(const PfQuat& q, float* R) {
    const double aa = q.a * q.a, bb = q.b * q.b, cc = q.c * q.c, dd = q.d * q.d;
    R[0] = (float)(aa + bb - cc - dd); R[1] = (float)(2.0 * (q.b * q.c - q.a * q.d)); R[2] = (float)(2.0 * (q.b * q.d + q.a * q.c));
    R[3] = (float)(2.0 * (q.b * q.c + q.a * q.d)); R[4] = (float)(aa - bb + cc - dd); R[5] = (float)(2.0 * (q.c * q.d - q.a * q.b));
    R[6] = (float)(2.0 * (q.b * q.d - q.a * q.c)); R[7] = (float)(2.0 * (q.c * q.d + q.a * q.b)); R[8] = (float)(aa - bb - cc + dd);
}
// the unit quaternion nearest to a matrix that is a rotation up to rounding (Shepperd: the largest of the four squares first)
PF_HD PfQuat pf_quat_of(const float* R) {
    const double m00 = R[0], m01 = R[1], m02 = R[2], m10 = R[3], m11 = R[4], m12 = R[5], m20 = R[6], m21 = R[7], m22 = R[8];
    const double ta = 1.0 + m00 + m11 + m22, tb = 1.0 + m00 - m11 - m22, tc = 1.0 - m00 + m11 - m22, td = 1.0 - m00 - m11 + m22;
    PfQuat q;
    if (ta >= tb && ta >= tc && ta >= td) { q.a = ta; q.b = m21 - m12; q.c = m02 - m20; q.d = m10 - m01; }
    else if (tb >= tc && tb >= td) { q.a = m21 - m12; q.b = tb; q.c = m01 + m10; q.d = m02 + m20; }
    else if (tc >= td) { q.a = m02 - m20; q.b = m01 + m10; q.c = tc; q.d = m12 + m21; }
    else { q.a = m10 - m01; q.b = m02 + m20; q.c = m12 + m21; q.d = td; }
    return pf_quat_unit(q);
}
// slerp(x, y, t) along the shorter arc; t = 0 gives x and t = 1 gives y bit for bit
PF_HD PfQuat pf_quat_slerp(const PfQuat& x, PfQuat y, double t) {
    if (t <= 0.0) return x;
    if (t >= 1.0) return y;
    double dot = (x.a * y.a + x.b * y.b) + (x.c * y.c + x.d * y.d);
    if (dot < 0.0) { dot = -dot; y.a = -y.a; y.b = -y.b; y.c = -y.c; y.d = -y.d; }
    double wx = 1.0 - t, wy = t;
    if (dot < 1.0 - 1e-12) {                                             // nearer than that the chord is the arc
        const double th = acos(dot), sn = sin(th);
        wx = sin((1.0 - t) * th) / sn; wy = sin(t * th) / sn;
    }
    PfQuat o;
    o.a = wx * x.a + wy * y.a; o.b = wx * x.b + wy * y.b; o.c = wx * x.c + wy * y.c; o.d = wx * x.d + wy * y.d;
    return pf_quat_unit(o);
}

// ---- solve -------------------------------------------------------------------------------------------------------------------
// one Jacobi rotation of the symmetric A (and of the eigenvector columns V) that zeroes A[p][q]; p, q are compile-time constants
// where it is called, so A and V stay in registers
#define PF_EGO_JACOBI(p, q)                                                                             \
    do {                                                                                                \
        const double apq = A[p][q];                                                                     \
        if (apq != 0.0) {                                                                               \
            const double th = (A[q][q] - A[p][p]) / (2.0 * apq);                                        \
            const double tt = (th < 0.0 ? -1.0 : 1.0) / (fabs(th) + sqrt(th * th + 1.0));               \
            const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;                                     \
            A[p][p] -= tt * apq; A[q][q] += tt * apq; A[p][q] = 0.0; A[q][p] = 0.0;                     \
            for (int k = 0; k < 4; ++k) {                                                               \
                if (k != p && k != q) {                                                                 \
                    const double akp = A[k][p], akq = A[k][q];                                          \
                    A[k][p] = c * akp - s * akq; A[p][k] = A[k][p];                                     \
                    A[k][q] = s * akp + c * akq; A[q][k] = A[k][q];                                     \
                }                                                                                       \
                const double vkp = V[k][p], vkq = V[k][q];                                              \
                V[k][p] = c * vkp - s * vkq; V[k][q] = s * vkp + c * vkq;                               \
            }                                                                                           \
        }                                                                                               \
    } while (0)

// image b: reads and zeroes its twelve sums, writes R (nine floats) and the five stats
PF_HD void pf_ego_solve_image(const PfEgoSolveArgs& a, int b) {
    long long* s = a.sums + (long)b * PF_EGO_SUMS;
    double S[9];
    for (int k = 0; k < 9; ++k) S[k] = (double)s[k] * a.inv;
    const double sw = (double)s[9] * a.inv, swr = (double)s[10] * a.inv_r, used = (double)s[11];
    for (int k = 0; k < PF_EGO_SUMS; ++k) s[k] = 0;
    const double Sxx = S[0], Sxy = S[1], Sxz = S[2], Syx = S[3], Syy = S[4], Syz = S[5], Szx = S[6], Szy = S[7], Szz = S[8];
    double A[4][4] = {{Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                      {Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz},
                      {Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy},
                      {Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz}};
    double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
    for (int sweep = 0; sweep < PF_EGO_SWEEPS; ++sweep) {
        PF_EGO_JACOBI(0, 1); PF_EGO_JACOBI(0, 2); PF_EGO_JACOBI(0, 3);
        PF_EGO_JACOBI(1, 2); PF_EGO_JACOBI(1, 3); PF_EGO_JACOBI(2, 3);
    }
    // the largest eigenvalue (ties to the earlier column) and the one after it, picked with constant indices
    double l1 = A[0][0];
    PfQuat e; e.a = V[0][0]; e.b = V[1][0]; e.c = V[2][0]; e.d = V[3][0];
    int i1 = 0;
    if (A[1][1] > l1) { l1 = A[1][1]; i1 = 1; e.a = V[0][1]; e.b = V[1][1]; e.c = V[2][1]; e.d = V[3][1]; }
    if (A[2][2] > l1) { l1 = A[2][2]; i1 = 2; e.a = V[0][2]; e.b = V[1][2]; e.c = V[2][2]; e.d = V[3][2]; }
    if (A[3][3] > l1) { l1 = A[3][3]; i1 = 3; e.a = V[0][3]; e.b = V[1][3]; e.c = V[2][3]; e.d = V[3][3]; }
    double l2 = -1.0e300;
    if (i1 != 0 && A[0][0] > l2) l2 = A[0][0];
    if (i1 != 1 && A[1][1] > l2) l2 = A[1][1];
    if (i1 != 2 && A[2][2] > l2) l2 = A[2][2];
    if (i1 != 3 && A[3][3] > l2) l2 = A[3][3];
    const bool some = sw > 0.0;
    const double gap = some ? (l1 - l2) / sw : 0.0;
    const bool valid = some && gap >= (double)a.gap_min;
    float* R = a.R + (long)b * 9;
    if (valid) {
        pf_quat_matrix(pf_quat_canon(e), R);
    } else {
        for (int k = 0; k < 9; ++k) R[k] = a.init ? a.init[(long)b * 9 + k] : (k % 4 == 0 ? 1.f : 0.f);
    }
    float* st = a.stats + (long)b * PF_EGO_STATS;
    st[0] = (float)sw;
    st[1] = some ? (float)sqrt(swr / sw) : 0.f;
    st[2] = (float)(used / ((double)a.H * (double)a.W));
    st[3] = (float)gap;
    st[4] = valid ? 1.f : 0.f;
}

// ---- tracking ----------------------------------------------------------------------------------------------------------------
// image b: state = {O, S} as two unit quaternions (fp64) with a >= 0.  O_t = R_t O_{t-1}, renormalised; S_t = slerp(S_{t-1}, O_t, t) with
// t = 1 - smoothing; orient = O_t and corr = O_t S_t^T as matrices
PF_HD void pf_ego_track_image(const PfEgoTrackArgs& a, int b) {
    double* st = a.state + (long)b * PF_EGO_STATE;
    PfQuat o, s;
    o.a = st[0]; o.b = st[1]; o.c = st[2]; o.d = st[3];
    s.a = st[4]; s.b = st[5]; s.c = st[6]; s.d = st[7];
    o = pf_quat_canon(pf_quat_mul(pf_quat_of(a.R + (long)b * 9), o));
    s = pf_quat_canon(pf_quat_slerp(s, o, a.t));
    st[0] = o.a; st[1] = o.b; st[2] = o.c; st[3] = o.d;
    st[4] = s.a; st[5] = s.b; st[6] = s.c; st[7] = s.d;
    pf_quat_matrix(o, a.orient + (long)b * 9);
    pf_quat_matrix(pf_quat_unit(pf_quat_mul(o, pf_quat_conj(s))), a.corr + (long)b * 9);
}

// ---- the two appliers --------------------------------------------------------------------------------------------------------
// out(x, y) = in sampled at erp(R s(x, y)): columns wrap, rows clamp.  Forms as pf_viewport_image: PF_VIEW_F32 [B,C,H,W] fp32,
// PF_VIEW_U8 [B,H,W,C] bytes (floor(x + 1/2) clamped to 0..255).  pix = y * W + x; cp, sp: pf_ego_row(y)
PF_HD void pf_erp_rotate_pixel(const PfErpRotArgs& a, const float* R, int b, int y, int x, float cp, float sp) {
    const PfVec3 p = pf_ego_p(x, a.W, cp, sp);
    float m, n;
    pf_vp_erp(pf_vp_rot(R, p.x, p.y, p.z), a.H, a.W, m, n);
    const PfWrapTaps t = pf_wraptaps(m, n, a.H, a.W);         // indices inside the map for any bits of R
    const long N = (long)a.H * a.W, pix = (long)y * a.W + x;
    if (a.form == PF_VIEW_F32) {
        const float* src = static_cast<const float*>(a.in) + (long)b * a.C * N;
        float* dst = static_cast<float*>(a.out) + (long)b * a.C * N + pix;
        for (int c = 0; c < a.C; ++c) {
            const float* s = src + c * N;
            dst[c * N] = pf_wrapmix(t, s[t.ia], s[t.ib], s[t.ic], s[t.id]);
        }
    } else {
        const long C = a.C;
        const unsigned char* src = static_cast<const unsigned char*>(a.in) + (long)b * N * C;
        unsigned char* dst = static_cast<unsigned char*>(a.out) + ((long)b * N + pix) * C;
        for (int c = 0; c < a.C; ++c)
            dst[c] = pf_vp_byte(pf_wrapmix(t, (float)src[t.ia * C + c], (float)src[t.ib * C + c], (float)src[t.ic * C + c],
                                           (float)src[t.id * C + c]));
    }
}
// flow'(x, y) = erp(R^T q) - (x, y), u' wrapped into [-W/2, W/2); a left-out pixel gives (0, 0) and valid 0
PF_HD void pf_ego_derotate_pixel(const PfEgoDerotArgs& a, const float* R, int b, int y, int x) {
    const long N = (long)a.H * a.W, n = (long)y * a.W + x;
    const float u = a.flow[((long)b * 2) * N + n], v = a.flow[((long)b * 2 + 1) * N + n];
    float ou = 0.f, ov = 0.f;
    unsigned char ok = 0;
    if (!pf_ego_left_out(u, v, a.mask ? a.mask[(long)b * N + n] : (unsigned char)0)) {
        float m, r;
        pf_vp_erp(pf_vp_rot_t(R, pf_ego_q(x, y, u, v, a.H, a.W)), a.H, a.W, m, r);
        const float Wf = (float)a.W;
        ou = pf_pymod((m - (float)x) + Wf * 0.5f, Wf) - Wf * 0.5f;
        ov = r - (float)y;
        ok = 1;
    }
    a.out[((long)b * 2) * N + n] = ou; a.out[((long)b * 2 + 1) * N + n] = ov;
    if (a.valid) a.valid[(long)b * N + n] = ok;
}

// ---- argument checks shared by the device entries and their host emulation ---------------------------------------------------
static inline int pf_ego_geometry(int B, int H, int W) {
    if (B < 1 || H < 1 || W < 1 || (long)H * W >= (1L << 30) || B > PF_EGO_MAX_GRID) return PF_ERR_BAD_SHAPE;
    return PF_OK;
}
static inline long pf_ego_bytes(int B, int H, int W) {
    const int rc = pf_ego_geometry(B, H, W);
    return rc != PF_OK ? rc : (long)B * PF_EGO_SUMS * 8;
}
static inline int pf_ego_accumulate_check(const float* flow, const unsigned char* mask, const float* R, void* sums, int B, int H,
                                          int W, int weighted, float scale_px, int blocks, PfEgoAccArgs& a) {
    if (!flow || !R || !sums || ((uintptr_t)sums & 7) || (const void*)flow == sums || (const void*)R == sums) return PF_ERR_BAD_ARG;
    if (weighted != 0 && weighted != 1) return PF_ERR_BAD_ARG;
    if (blocks < 0 || blocks > PF_EGO_MAX_GRID) return PF_ERR_BAD_ARG;
    const int rc = pf_ego_geometry(B, H, W);
    if (rc != PF_OK) return rc;
    const float c = scale_px * (PF_VP_TWO_PI / (float)W);
    const float inv_c2 = 1.f / (c * c);
    if (!(scale_px > 0.f && pf_finite(scale_px) && pf_finite(inv_c2) && inv_c2 > 0.f)) return PF_ERR_BAD_ARG;
    const PfEgoScales s = pf_ego_scales(H, W);
    a.flow = flow; a.mask = mask; a.R = R; a.sums = static_cast<long long*>(sums); a.B = B; a.H = H; a.W = W; a.weighted = weighted;
    a.inv_c2 = inv_c2; a.f = s.f; a.fr = s.fr;
    return PF_OK;
}
static inline int pf_ego_solve_check(void* sums, const float* init, float* R, float* stats, int B, int H, int W, float gap_min,
                                     PfEgoSolveArgs& a) {
    if (!sums || !R || !stats || ((uintptr_t)sums & 7) || (void*)R == sums || (void*)stats == sums || R == stats || stats == init)
        return PF_ERR_BAD_ARG;
    if (!(gap_min >= 0.f && pf_finite(gap_min))) return PF_ERR_BAD_ARG;
    const int rc = pf_ego_geometry(B, H, W);
    if (rc != PF_OK) return rc;
    const PfEgoScales s = pf_ego_scales(H, W);
    a.sums = static_cast<long long*>(sums); a.init = init; a.R = R; a.stats = stats; a.B = B; a.H = H; a.W = W; a.gap_min = gap_min;
    a.inv = s.inv; a.inv_r = s.inv_r;
    return PF_OK;
}
static inline int pf_ego_track_check(const float* R, void* state, float* orient, float* corr, int B, float smoothing, PfEgoTrackArgs& a) {
    if (!R || !state || !orient || !corr || ((uintptr_t)state & 7) || orient == corr || orient == R || corr == R
        || state == (void*)orient || state == (void*)corr || state == (const void*)R) return PF_ERR_BAD_ARG;
    if (!(smoothing >= 0.f && smoothing <= 1.f)) return PF_ERR_BAD_ARG;
    if (B < 1 || B > PF_EGO_MAX_GRID) return PF_ERR_BAD_SHAPE;
    a.R = R; a.state = static_cast<double*>(state); a.orient = orient; a.corr = corr; a.B = B; a.t = 1.0 - (double)smoothing;
    return PF_OK;
}
static inline int pf_erp_rotate_check(const void* in, void* out, const float* R, int B, int C, int H, int W, int form, PfErpRotArgs& a) {
    if (!in || !out || !R || in == out || (const void*)R == in || (const void*)R == out) return PF_ERR_BAD_ARG;
    if (form != PF_VIEW_F32 && form != PF_VIEW_U8) return PF_ERR_BAD_ARG;
    if (C < 1 || C > 4) return PF_ERR_BAD_ARG;
    const int rc = pf_ego_geometry(B, H, W);
    if (rc != PF_OK) return rc;
    a.in = in; a.out = out; a.R = R; a.B = B; a.C = C; a.H = H; a.W = W; a.form = form;
    return PF_OK;
}
static inline int pf_ego_derotate_check(const float* flow, const unsigned char* mask, const float* R, float* out, unsigned char* valid,
                                        int B, int H, int W, PfEgoDerotArgs& a) {
    if (!flow || !R || !out || (const void*)R == (const void*)out || (const void*)valid == (const void*)out
        || (valid && ((const void*)valid == (const void*)flow || valid == mask)) || (mask && (const void*)mask == (const void*)out))
        return PF_ERR_BAD_ARG;
    const int rc = pf_ego_geometry(B, H, W);
    if (rc != PF_OK) return rc;
    a.flow = flow; a.mask = mask; a.R = R; a.out = out; a.valid = valid; a.B = B; a.H = H; a.W = W;
    return PF_OK;
}
