// Camera translation from a full-sphere flow field: the epipole, inverse depth up to the baseline and a mask of what moves against
// the static scene (include/priorflow_hip.h: pf_epi_accumulate, pf_epi_solve, pf_epi_map).  The statement,
// once, for the device kernels (pf_epipolar.hip), the host emulation (tests/emu/pf_emu_epipolar.cpp) and the C checks.  The
// bearings p and q, the left-out rule, the quantisation, the scales and the quaternions are pf_egomotion.h's; nothing of them is
// restated here.
//
// Model: q ~ R p + kappa t, t a unit vector, kappa = |T| / depth >= 0.  This is the POINT-motion convention: a point of the scene
// moves by T = |T| t in the second frame's axes; the camera centre moves along -R^T t in the first frame's.
//
// Pixel (x, y) of image b, every step a rounded fp32 operation, with r = R p:
//   n = r x q                                the normal of the pixel's epipolar plane; a static pixel has t . n = 0
//   n^ = n / sqrt(|n|^2 + c_v^2)             its VOTE, c_v = vote_px 2 pi / W: a large displacement counts as one unit vote, a tiny one
//                                            in proportion to its size (without it a moving object of a few pixels outweighs sub-pixel
//                                            parallax by its square and the reweighting never recovers)
//   m = t x r,  e = (q . m) / |m| when |m|^2 >= 1e-12, else 0: the distance of q from the epipolar great circle of r under the
//                                            current t; a pixel at the epipole, and every pixel while t = 0, agrees with anything
//   e^2 is clamped to 1, NaN included, so whatever t and R in memory hold the weight lies in [0, 1]
//   w = cos phi(y) g,  g = 1 / (1 + e^2 / c^2)^2,  c = scale_px 2 pi / W  (g = 1 when t = 0)
//   d = (q - r) - ((q - r) . r) r            the displacement in r's tangent plane: sum w d . t > 0 for positive depths, whatever
//                                            t the pass started from
//   e_a = t . n,  g_w = (t . r) q - (r . q) t: to first order e_a + dw . g_w = 0 under R <- exp([dw]x) R
//
// PF_EPI_SUMS = 22 sums per image, 64-bit integers, a contribution pf_ego_quant(value, 2^S') of the fp32 value, so the adds
// commute and the result is the same bits on every run and for every grid.  pf_ego_scales(H, W) is the one source of the scales:
// S for values bounded by 1, S - 2 for values bounded by 4.
//   T pass (mode PF_EPI_T):  0..5  M = sum w n^ n^T (xx xy xz yy yz zz)    S     |n^| < 1
//                            6..8  D = sum w d                             S-2   |d| <= |q - r| <= 2
//                            9     sum w                                   S
//                            10    sum w e^2                               S     e^2 <= 1
//                            11    sum w min(|n|^2, 4)                     S-2   (1 for a rotation R; the clamp covers any bits of R)
//                            12    the number of pixels used
//   R pass (mode PF_EPI_R):  13..18 G = sum w g_w g_w^T (xx xy xz yy yz zz) S-2  |g_w| <= 2, entries <= 4
//                            19..21 h = sum w e_a g_w                       S-2  |e_a| <= 1, |g_w| <= 2
//                            9, 12 as above
// A pass adds only to the sums its solve reads.  Worst case, as in pf_egomotion.h: every one of the H W pixels at the maximum adds
// 2^S <= 2^62 / (H W) (a value bounded by 4 at 2^(S-2) the same), a sum of at most 2^62; the H W roundings of at most 1/2 each
// and the few ulp by which fp32 bearings exceed a unit length do not reach the remaining bit.  The bounds hold for R a rotation
// up to rounding and |t| <= 1; whatever the two hold, no address depends on them.
//
// Solve, per image, in fp64, one lane per image, writing zeros over the sums it read:
//   T: 3 x 3 cyclic Jacobi on M (PF_EPI_JACOBI, compile-time indices); t = the unit eigenvector of the smallest eigenvalue, its
//      sign flipped when t . D < 0.  stats [B,6] = {sum w, rms e in pixel widths, used / (H W), gap = (l2 - l1) / (l1 + l2 + l3),
//      parallax rms sqrt(sum w |n|^2 / sum w) in pixel widths, valid}; valid = 0 when sum w = 0, gap < gap_min or the parallax rms
//      < min_parallax_px (a pure rotation has no epipole), and then t is t_init, or the zero vector without one.
//   R: dw = -G^-1 h by the same Jacobi; dw = 0 when the T solve before it was not valid (stats[5] == 0: a fit without an epipole
//      must not touch the rotation), when t = 0, or when the smallest eigenvalue of G is below 1e-9 of its trace;
//      R <- exp([dw]x) R through the quaternions, in place (R is left bit for bit when dw = 0).
//
// Map, per pixel, every output optional: conf = |q x t|^2, the signed parallax a = (r x q) . (q x t) / |q x t|, kappa = a / |q x t|,
// resid = |e| in pixel widths, moving = resid > thr_px or a < -neg_px 2 pi / W.  A left-out pixel, a pixel with conf < conf_min,
// or t = 0 gives kappa = 0, resid = 0, conf as computed (0 when left out) and moving = 0.  Nothing is indexed by a flow value.
#pragma once
#include "pf_egomotion.h"

#define PF_EPI_TINY 1e-12f
static_assert(PF_EPI_SUMS == 22 && PF_EPI_STATS == 6, "the sizes of pf_epipolar.h and of the public header");

struct PfEpiAccArgs {
    const float* flow; const unsigned char* mask; const float* R; const float* t;      // [B,2,H,W], [B,H,W] or null, [B,9], [B,3] or null
    long long* sums;                                                                     // [B,22]
    int B, H, W, mode; float inv_c2, cv2, f, fr;
};
struct PfEpiSolveArgs {
    long long* sums; const float* t_init; float* R; float* t; float* stats;
    int B, H, W, mode; float gap_min, min_parallax_px; double inv, inv_r;
};
struct PfEpiMapArgs {
    const float* flow; const unsigned char* mask; const float* R; const float* t;
    float* inv_depth; float* resid; float* conf; unsigned char* moving;
    int B, H, W; float thr_px, neg, conf_min, px;                                        // neg = neg_px 2 pi / W, px = W / 2 pi
};

PF_HD PfVec3 pf_epi_cross(const PfVec3& a, const PfVec3& b) {
    PfVec3 c; c.x = a.y * b.z - a.z * b.y; c.y = a.z * b.x - a.x * b.z; c.z = a.x * b.y - a.y * b.x; return c;
}
PF_HD float pf_epi_dot(const PfVec3& a, const PfVec3& b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
// e = (q . (t x r)) / |t x r|, 0 at the epipole and while t = 0
PF_HD float pf_epi_resid(const PfVec3& t, const PfVec3& r, const PfVec3& q) {
    const PfVec3 m = pf_epi_cross(t, r);
    const float mm = pf_epi_dot(m, m);
    return mm >= PF_EPI_TINY ? pf_epi_dot(q, m) / sqrtf(mm) : 0.f;
}

// pixel (x, y) with flow (u, v) and mask byte m into the partial sums s[PF_EPI_SUMS] of its MODE; cp, sp: pf_ego_row(y); R, t: the
// image's current rotation and translation
template <int MODE>
PF_HD void pf_epi_pixel(const PfEpiAccArgs& a, const float* R, const PfVec3& t, float cp, float sp, int y, int x, float u, float v,
                        unsigned char m, long long* s) {
    if (pf_ego_left_out(u, v, m)) return;
    const PfVec3 p = pf_ego_p(x, a.W, cp, sp), q = pf_ego_q(x, y, u, v, a.H, a.W);
    const PfVec3 r = pf_vp_rot(R, p.x, p.y, p.z);
    const PfVec3 n = pf_epi_cross(r, q);
    const float e = pf_epi_resid(t, r, q);
    float e2 = e * e;
    e2 = e2 <= 1.f ? e2 : 1.f;                                            // a NaN takes the clamp
    const float g1 = 1.f + e2 * a.inv_c2;
    const float w = cp * (1.f / (g1 * g1));
    s[9] += pf_ego_quant(w, a.f);
    s[12] += 1;
    if (MODE == PF_EPI_T) {
        float nn = pf_epi_dot(n, n);
        const float inv = 1.f / sqrtf(nn + a.cv2);
        const float hx = n.x * inv, hy = n.y * inv, hz = n.z * inv;
        const float wx = w * hx, wy = w * hy, wz = w * hz;
        s[0] += pf_ego_quant(wx * hx, a.f); s[1] += pf_ego_quant(wx * hy, a.f); s[2] += pf_ego_quant(wx * hz, a.f);
        s[3] += pf_ego_quant(wy * hy, a.f); s[4] += pf_ego_quant(wy * hz, a.f); s[5] += pf_ego_quant(wz * hz, a.f);
        const float dx = q.x - r.x, dy = q.y - r.y, dz = q.z - r.z;
        const float dr = (dx * r.x + dy * r.y) + dz * r.z;
        s[6] += pf_ego_quant(w * (dx - dr * r.x), a.fr); s[7] += pf_ego_quant(w * (dy - dr * r.y), a.fr);
        s[8] += pf_ego_quant(w * (dz - dr * r.z), a.fr);
        s[10] += pf_ego_quant(w * e2, a.f);
        nn = nn <= 4.f ? nn : 4.f;
        s[11] += pf_ego_quant(w * nn, a.fr);
    } else {
        const float ea = pf_epi_dot(t, n), tr = pf_epi_dot(t, r), rq = pf_epi_dot(r, q);
        const float gx = tr * q.x - rq * t.x, gy = tr * q.y - rq * t.y, gz = tr * q.z - rq * t.z;
        const float wx = w * gx, wy = w * gy, wz = w * gz;
        s[13] += pf_ego_quant(wx * gx, a.fr); s[14] += pf_ego_quant(wx * gy, a.fr); s[15] += pf_ego_quant(wx * gz, a.fr);
        s[16] += pf_ego_quant(wy * gy, a.fr); s[17] += pf_ego_quant(wy * gz, a.fr); s[18] += pf_ego_quant(wz * gz, a.fr);
        s[19] += pf_ego_quant(wx * ea, a.fr); s[20] += pf_ego_quant(wy * ea, a.fr); s[21] += pf_ego_quant(wz * ea, a.fr);
    }
}

// ---- solve -------------------------------------------------------------------------------------------------------------------
// PF_EGO_JACOBI in three dimensions: one rotation of the symmetric A (and of the eigenvector columns V) that zeroes A[p][q]
#define PF_EPI_JACOBI(p, q)                                                                             \
    do {                                                                                                \
        const double apq = A[p][q];                                                                     \
        if (apq != 0.0) {                                                                               \
            const double th = (A[q][q] - A[p][p]) / (2.0 * apq);                                        \
            const double tt = (th < 0.0 ? -1.0 : 1.0) / (fabs(th) + sqrt(th * th + 1.0));               \
            const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;                                     \
            A[p][p] -= tt * apq; A[q][q] += tt * apq; A[p][q] = 0.0; A[q][p] = 0.0;                     \
            for (int k = 0; k < 3; ++k) {                                                               \
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
// the eigenvalues (A's diagonal afterwards) and eigenvectors (V's columns) of the symmetric matrix {xx xy xz yy yz zz}
#define PF_EPI_EIGEN(m6)                                                                                \
    double A[3][3] = {{m6[0], m6[1], m6[2]}, {m6[1], m6[3], m6[4]}, {m6[2], m6[4], m6[5]}};             \
    double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};                                                 \
    for (int sweep = 0; sweep < PF_EGO_SWEEPS; ++sweep) { PF_EPI_JACOBI(0, 1); PF_EPI_JACOBI(0, 2); PF_EPI_JACOBI(1, 2); }

// image b, T solve: reads and zeroes sums 0..12, writes t (three floats) and the six stats
PF_HD void pf_epi_solve_t_image(const PfEpiSolveArgs& a, int b) {
    long long* s = a.sums + (long)b * PF_EPI_SUMS;
    double M[6], D[3];
    for (int k = 0; k < 6; ++k) M[k] = (double)s[k] * a.inv;
    for (int k = 0; k < 3; ++k) D[k] = (double)s[6 + k] * a.inv_r;
    const double sw = (double)s[9] * a.inv, swe = (double)s[10] * a.inv, swn = (double)s[11] * a.inv_r, used = (double)s[12];
    for (int k = 0; k <= 12; ++k) s[k] = 0;
    PF_EPI_EIGEN(M)
    // the smallest eigenvalue (ties to the earlier column), picked with constant indices, and the one after it
    double l1 = A[0][0], vx = V[0][0], vy = V[1][0], vz = V[2][0];
    int i1 = 0;
    if (A[1][1] < l1) { l1 = A[1][1]; i1 = 1; vx = V[0][1]; vy = V[1][1]; vz = V[2][1]; }
    if (A[2][2] < l1) { l1 = A[2][2]; i1 = 2; vx = V[0][2]; vy = V[1][2]; vz = V[2][2]; }
    double l2 = 1.0e300;
    if (i1 != 0 && A[0][0] < l2) l2 = A[0][0];
    if (i1 != 1 && A[1][1] < l2) l2 = A[1][1];
    if (i1 != 2 && A[2][2] < l2) l2 = A[2][2];
    const double trace = (A[0][0] + A[1][1]) + A[2][2];
    const bool some = sw > 0.0;
    const double px = (double)a.W / 6.283185307179586;
    const double gap = (some && trace > 0.0) ? (l2 - l1) / trace : 0.0;
    const double par = some ? px * sqrt(swn / sw) : 0.0;
    const bool valid = some && gap >= (double)a.gap_min && par >= (double)a.min_parallax_px;
    float* t = a.t + (long)b * 3;
    if (valid) {
        const double nrm = sqrt((vx * vx + vy * vy) + vz * vz);
        const double sg = ((vx * D[0] + vy * D[1]) + vz * D[2]) < 0.0 ? -1.0 / nrm : 1.0 / nrm;
        t[0] = (float)(vx * sg); t[1] = (float)(vy * sg); t[2] = (float)(vz * sg);
    } else {
        for (int k = 0; k < 3; ++k) t[k] = a.t_init ? a.t_init[(long)b * 3 + k] : 0.f;
    }
    float* st = a.stats + (long)b * PF_EPI_STATS;
    st[0] = (float)sw;
    st[1] = some ? (float)(px * sqrt(swe / sw)) : 0.f;
    st[2] = (float)(used / ((double)a.H * (double)a.W));
    st[3] = (float)gap;
    st[4] = (float)par;
    st[5] = valid ? 1.f : 0.f;
}

// image b, R solve: reads and zeroes sums 9, 12, 13..21, reads t and stats[5], updates R in place
PF_HD void pf_epi_solve_r_image(const PfEpiSolveArgs& a, int b) {
    long long* s = a.sums + (long)b * PF_EPI_SUMS;
    double G[6], h[3];
    for (int k = 0; k < 6; ++k) G[k] = (double)s[13 + k] * a.inv_r;
    for (int k = 0; k < 3; ++k) h[k] = (double)s[19 + k] * a.inv_r;
    s[9] = 0; s[12] = 0;
    for (int k = 13; k < PF_EPI_SUMS; ++k) s[k] = 0;
    const float* t = a.t + (long)b * 3;
    const bool have_t = a.stats[(long)b * PF_EPI_STATS + 5] != 0.f && (t[0] != 0.f || t[1] != 0.f || t[2] != 0.f);
    PF_EPI_EIGEN(G)
    const double trace = (A[0][0] + A[1][1]) + A[2][2];
    double lmin = A[0][0];
    if (A[1][1] < lmin) lmin = A[1][1];
    if (A[2][2] < lmin) lmin = A[2][2];
    if (!(have_t && trace > 0.0 && lmin >= 1e-9 * trace)) return;        // a NaN leaves R as it is
    // dw = -sum_k v_k (v_k . h) / lambda_k
    const double c0 = ((V[0][0] * h[0] + V[1][0] * h[1]) + V[2][0] * h[2]) / A[0][0];
    const double c1 = ((V[0][1] * h[0] + V[1][1] * h[1]) + V[2][1] * h[2]) / A[1][1];
    const double c2 = ((V[0][2] * h[0] + V[1][2] * h[1]) + V[2][2] * h[2]) / A[2][2];
    const double wx = -((V[0][0] * c0 + V[0][1] * c1) + V[0][2] * c2);
    const double wy = -((V[1][0] * c0 + V[1][1] * c1) + V[1][2] * c2);
    const double wz = -((V[2][0] * c0 + V[2][1] * c1) + V[2][2] * c2);
    const double th = sqrt((wx * wx + wy * wy) + wz * wz);
    if (!(th > 0.0)) return;
    const double k = sin(0.5 * th) / th;
    PfQuat dq; dq.a = cos(0.5 * th); dq.b = k * wx; dq.c = k * wy; dq.d = k * wz;
    float* R = a.R + (long)b * 9;
    pf_quat_matrix(pf_quat_canon(pf_quat_mul(dq, pf_quat_of(R))), R);
}
PF_HD void pf_epi_solve_image(const PfEpiSolveArgs& a, int b) {
    if (a.mode == PF_EPI_T) pf_epi_solve_t_image(a, b); else pf_epi_solve_r_image(a, b);
}

// ---- map ---------------------------------------------------------------------------------------------------------------------
PF_HD void pf_epi_map_pixel(const PfEpiMapArgs& a, const float* R, const PfVec3& t, int b, int y, int x) {
    const long N = (long)a.H * a.W, n = (long)y * a.W + x;
    const float u = a.flow[((long)b * 2) * N + n], v = a.flow[((long)b * 2 + 1) * N + n];
    float kappa = 0.f, resid = 0.f, conf = 0.f;
    unsigned char moving = 0;
    if (!pf_ego_left_out(u, v, a.mask ? a.mask[(long)b * N + n] : (unsigned char)0)) {
        float cp, sp;
        pf_ego_row(y, a.H, cp, sp);
        const PfVec3 p = pf_ego_p(x, a.W, cp, sp), q = pf_ego_q(x, y, u, v, a.H, a.W);
        const PfVec3 r = pf_vp_rot(R, p.x, p.y, p.z);
        const PfVec3 qt = pf_epi_cross(q, t);
        conf = pf_epi_dot(qt, qt);
        if (conf >= a.conf_min && conf > 0.f) {                             // t = 0 has conf = 0; a NaN compares false
            const float len = sqrtf(conf);
            const float par = pf_epi_dot(pf_epi_cross(r, q), qt) / len;
            kappa = par / len;
            resid = fabsf(pf_epi_resid(t, r, q)) * a.px;
            moving = (resid > a.thr_px || par < -a.neg) ? 1 : 0;
        }
    }
    const long o = (long)b * N + n;
    if (a.inv_depth) a.inv_depth[o] = kappa;
    if (a.resid) a.resid[o] = resid;
    if (a.conf) a.conf[o] = conf;
    if (a.moving) a.moving[o] = moving;
}

// ---- argument checks shared by the device entries and their host emulation ---------------------------------------------------
static inline long pf_epi_bytes(int B, int H, int W) {
    const int rc = pf_ego_geometry(B, H, W);
    return rc != PF_OK ? rc : (long)B * PF_EPI_SUMS * 8;
}
static inline bool pf_epi_scale_ok(float px, int W, float& inv2) {
    const float c = px * (PF_VP_TWO_PI / (float)W);
    inv2 = 1.f / (c * c);
    return px > 0.f && pf_finite(px) && pf_finite(inv2) && inv2 > 0.f;
}
static inline int pf_epi_accumulate_check(const float* flow, const unsigned char* mask, const float* R, const float* t, void* sums,
                                          int B, int H, int W, int mode, float scale_px, float vote_px, int blocks, PfEpiAccArgs& a) {
    if (!flow || !R || !sums || ((uintptr_t)sums & 7) || (const void*)flow == sums || (const void*)R == sums
        || (const void*)t == sums || (t && t == R)) return PF_ERR_BAD_ARG;
    if (mode != PF_EPI_T && mode != PF_EPI_R) return PF_ERR_BAD_ARG;
    if (mode == PF_EPI_R && !t) return PF_ERR_BAD_ARG;                    // the refinement turns about a translation
    if (blocks < 0 || blocks > PF_EGO_MAX_GRID) return PF_ERR_BAD_ARG;
    const int rc = pf_ego_geometry(B, H, W);
    if (rc != PF_OK) return rc;
    float inv_c2, inv_cv2;
    if (!pf_epi_scale_ok(scale_px, W, inv_c2) || !pf_epi_scale_ok(vote_px, W, inv_cv2)) return PF_ERR_BAD_ARG;
    const float cv = vote_px * (PF_VP_TWO_PI / (float)W);
    if (!(cv * cv > 0.f)) return PF_ERR_BAD_ARG;
    const PfEgoScales s = pf_ego_scales(H, W);
    a.flow = flow; a.mask = mask; a.R = R; a.t = t; a.sums = static_cast<long long*>(sums); a.B = B; a.H = H; a.W = W; a.mode = mode;
    a.inv_c2 = inv_c2; a.cv2 = cv * cv; a.f = s.f; a.fr = s.fr;
    return PF_OK;
}
static inline int pf_epi_solve_check(void* sums, const float* t_init, float* R, float* t, float* stats, int B, int H, int W, int mode,
                                     float gap_min, float min_parallax_px, PfEpiSolveArgs& a) {
    if (!sums || !t || !stats || ((uintptr_t)sums & 7) || (void*)t == sums || (void*)stats == sums || (void*)R == sums || t == stats
        || t == t_init || stats == t_init || (R && (R == t || R == stats || R == t_init))) return PF_ERR_BAD_ARG;
    if (mode != PF_EPI_T && mode != PF_EPI_R) return PF_ERR_BAD_ARG;
    if (mode == PF_EPI_R && !R) return PF_ERR_BAD_ARG;
    if (!(gap_min >= 0.f && pf_finite(gap_min) && min_parallax_px >= 0.f && pf_finite(min_parallax_px))) return PF_ERR_BAD_ARG;
    const int rc = pf_ego_geometry(B, H, W);
    if (rc != PF_OK) return rc;
    const PfEgoScales s = pf_ego_scales(H, W);
    a.sums = static_cast<long long*>(sums); a.t_init = t_init; a.R = R; a.t = t; a.stats = stats; a.B = B; a.H = H; a.W = W;
    a.mode = mode; a.gap_min = gap_min; a.min_parallax_px = min_parallax_px; a.inv = s.inv; a.inv_r = s.inv_r;
    return PF_OK;
}
static inline int pf_epi_map_check(const float* flow, const unsigned char* mask, const float* R, const float* t, float* inv_depth,
                                   float* resid, float* conf, unsigned char* moving, int B, int H, int W, float thr_px, float neg_px,
                                   float conf_min, PfEpiMapArgs& a) {
    if (!flow || !R || !t || R == t) return PF_ERR_BAD_ARG;
    const void* outs[4] = {inv_depth, resid, conf, moving};
    for (int i = 0; i < 4; ++i) {
        if (!outs[i]) continue;
        if (outs[i] == (const void*)flow || outs[i] == (const void*)mask || outs[i] == (const void*)R || outs[i] == (const void*)t)
            return PF_ERR_BAD_ARG;
        for (int j = 0; j < i; ++j) if (outs[j] == outs[i]) return PF_ERR_BAD_ARG;
    }
    if (!(thr_px >= 0.f && pf_finite(thr_px) && neg_px >= 0.f && pf_finite(neg_px) && conf_min >= 0.f && pf_finite(conf_min)))
        return PF_ERR_BAD_ARG;
    const int rc = pf_ego_geometry(B, H, W);
    if (rc != PF_OK) return rc;
    a.flow = flow; a.mask = mask; a.R = R; a.t = t; a.inv_depth = inv_depth; a.resid = resid; a.conf = conf; a.moving = moving;
    a.B = B; a.H = H; a.W = W; a.thr_px = thr_px; a.neg = neg_px * (PF_VP_TWO_PI / (float)W); a.conf_min = conf_min;
    a.px = (float)W / PF_VP_TWO_PI;
    return PF_OK;
}
