// Camera trajectory from 360-degree video: the scale link between consecutive pairs, the pose chain and depth fused in one unit
// (include/priorflow_hip.h: pf_odo_accumulate, pf_odo_solve, pf_odo_reverse_pose, pf_odo_track,
// pf_odo_fuse).  The statement, once, for the device kernels (pf_odometry.hip), the host emulation
// (tests/emu/pf_emu_odometry.cpp) and the C checks.  The quantisation, the scales, cos phi of a row and the quaternions are
// pf_egomotion.h's, the maps are what pf_epipolar.h's pf_epi_map_pixel writes; nothing of them is restated here.
//
// Two parallax maps on ONE grid, the grid of the frame two consecutive pairs share: map a = (kappa_a, conf_a, moving_a) of the
// earlier pair's backward flow under its reversed pose, kappa_a = |T_k| / rho; map b of the later pair's forward flow,
// kappa_b = |T_k+1| / rho, rho the depth of the same point in the same frame.  kappa_b / kappa_a = |T_k+1| / |T_k| at every
// static pixel.
//
// Link pixel (x, y), every step a rounded fp32 operation.  LEFT OUT when a moving byte is non-zero, !(conf > 0) for either map or
// !(kappa >= kappa_min && kappa < 2^30) for either map (a NaN compares false); those tests come before any other use.  Else
//   w   = (cos phi(y) min(conf_a, 1)) min(conf_b, 1)                                     in [0, 1]
//   l   = log2f(kappa_b / kappa_a),  l_c = l clamped to [-L, L]                          L = log2_range
//   bin = floor(((l_c + L) bins) / (2 L)) clamped to [0, bins - 1]
// Nothing is indexed by an input value before it has passed the tests, and the bin is clamped after them.
//
// Histogram, per image 2 bins + 2 cells of 64-bit integers (PF_ODO_CELLS(bins)), contributions pf_ego_quant(value, 2^S) with
// S = pf_ego_scales(H, W).s, so the adds commute and the result is the same bits on every run and for every grid:
//   W[bin] += quant(w)                 cells 0 .. bins - 1
//   M[bin] += quant((w l_c) / L)       cells bins .. 2 bins - 1      |w l_c / L| <= 1
//   total  += quant(w)                 cell 2 bins
//   count  += 1                        cell 2 bins + 1
// Worst case as in pf_egomotion.h: H W pixels that each add 2^S <= 2^62 / (H W) to ONE cell, a sum of at most 2^62.
//
// Solve, per image, on the integers (so the answer is the same for any order of the adds), one lane per image:
//   total = sum W.  With the inclusive prefix sum C, the median bin m is the smallest with 2 C >= total, q1 with 4 C >= total, q3
//   with 4 C >= 3 total (compared as C >= ceil(total k / 4) in unsigned 64-bit arithmetic: 3 * 2^62 + 3 < 2^64).
//   window = [m - trim_bins, m + trim_bins] cut to [0, bins - 1];  l^ = L sum M / sum W over the window, in fp64;
//   ratio = (float)exp2(l^).  stats [B,6] = {total 2^-S, used / (H W), l^, iqr = (q3 - q1) 2 L / bins, window weight / total, valid}
//   valid = 0 and ratio = 1 when total <= 0, used / (H W) < min_used, iqr > max_iqr, or m is bin 0 or bin bins - 1 (the clamp bins).
//   The solve writes zeros over every cell.
//
// Reverse pose: (R, t) -> (R^T, -R^T t); the components are 0 - (...) so that t = 0 stays +0.
//
// Track, per image an fp64 state of PF_ODO_STATE = 12 values {A (unit quaternion, a >= 0), b[3], S, steps, segment, prev_valid, 0}
// ({1,0,0,0, 0,0,0, 1, 0,0,0, 0} at the start): X_k = A_k X_0 + b_k in the axes of the first frame.  A step with the pair's R, t,
// pose valid pv, the link's ratio and valid flag lv:
//   A <- canon(q(R) A);  b <- R b;
//   pv and prev_valid and lv:  S <- S ratio;     pv otherwise: S stays, segment += 1 (the first valid pair opens segment 1)
//   pv: b <- b + S t;     prev_valid <- pv;  steps += 1
// A pair without an observable translation turns the camera and breaks the chain.  Out: orientation = matrix(A), centre =
// -A^T b, baseline S (fp32), flags int32 {steps, segment, pv, lv}.
//
// Fuse pixel: a map counts where its moving byte is 0, conf >= conf_min and 0 <= kappa < 2^30 (map a only where link_valid != 0);
// its weight is then conf, else 0.  d = kappa / S; inv_depth = (w_a d_a + w_b d_b) / (w_a + w_b), weight = w_a + w_b, both 0 where
// nothing counts or the weight sum is not positive and finite; disagree = both count, both kappa >= kappa_min and |log2f(d_b / d_a)| > tol_log2.  Every element of every output is
// written; every output is optional.  S_a, S_b, link_valid are DEVICE scalars [B].
#pragma once
#include "pf_egomotion.h"
#include "pf_epipolar.h"

#define PF_ODO_CELLS(bins) (2 * (bins) + 2)
static_assert(PF_ODO_STATS == 6 && PF_ODO_STATE == 12 && PF_ODO_FLAGS == 4, "the sizes of pf_odometry.h and of the public header");

struct PfOdoMap { const float* inv; const float* conf; const unsigned char* moving; };     // [B,H,W] each
struct PfOdoAccArgs {
    PfOdoMap a, b; long long* hist;                                                       // [B, 2 bins + 2]
    int B, H, W, bins; float L, two_L, binsf, kappa_min, f;
};
struct PfOdoSolveArgs {
    long long* hist; float* ratio; float* stats;                                          // [B], [B,6]
    int B, H, W, bins, trim; float min_used, max_iqr; double L, inv;
};
struct PfOdoReverseArgs { const float* R; const float* t; float* Rr; float* tr; int B; };
struct PfOdoTrackArgs {
    const float* R; const float* t; const float* pose_stats; const float* ratio; const float* link_stats;
    double* state; float* orient; float* centre; float* baseline; int* flags; int B;
};
struct PfOdoFuseArgs {
    PfOdoMap a, b; const float* S_a; const float* S_b; const float* link_valid;
    float* inv_depth; float* weight; unsigned char* disagree;
    int B, H, W; float conf_min, kappa_min, tol;
};

// ---- link --------------------------------------------------------------------------------------------------------------------
PF_HD bool pf_odo_kappa_ok(float k, float kmin) { return k >= kmin && k < PF_EGO_FAR; }
// false: the pixel is left out.  cp: cos phi of the row (pf_ego_row).  -> bin in [0, bins - 1], the weight and l_c
PF_HD bool pf_odo_link_pixel(const PfOdoAccArgs& a, float cp, float ka, float ca, unsigned char ma, float kb, float cb, unsigned char mb,
                             int& bin, float& w, float& lc) {
    if (ma != 0 || mb != 0) return false;
    if (!(ca > 0.f) || !(cb > 0.f)) return false;
    if (!pf_odo_kappa_ok(ka, a.kappa_min) || !pf_odo_kappa_ok(kb, a.kappa_min)) return false;
    w = (cp * (ca < 1.f ? ca : 1.f)) * (cb < 1.f ? cb : 1.f);
    const float l = log2f(kb / ka);
    lc = l < -a.L ? -a.L : (l > a.L ? a.L : l);
    const float pos = floorf(((lc + a.L) * a.binsf) / a.two_L);
    int k = (int)pos;                                                    // pos in [0, bins]: lc is finite and inside the range
    bin = k < 0 ? 0 : (k > a.bins - 1 ? a.bins - 1 : k);
    return true;
}
// the two contributions of a pixel that counts
PF_HD long long pf_odo_qw(const PfOdoAccArgs& a, float w) { return pf_ego_quant(w, a.f); }
PF_HD long long pf_odo_qm(const PfOdoAccArgs& a, float w, float lc) { return pf_ego_quant((w * lc) / a.L, a.f); }

// ---- solve -------------------------------------------------------------------------------------------------------------------
PF_HD void pf_odo_solve_image(const PfOdoSolveArgs& a, int b) {
    const int bins = a.bins;
    long long* h = a.hist + (long)b * PF_ODO_CELLS(bins);
    unsigned long long total = 0;
    bool sane = true;                                                     // a cell below zero: leftovers, not a histogram
    for (int k = 0; k < bins; ++k) { sane = sane && h[k] >= 0; total += (unsigned long long)h[k]; }
    sane = sane && total > 0 && total <= (1ULL << 62);
    const double sw = (double)h[2 * bins] * a.inv, used = (double)h[2 * bins + 1] / ((double)a.H * (double)a.W);
    int m = 0, q1 = 0, q3 = 0;
    double lhat = 0.0, share = 0.0;
    if (sane) {
        const unsigned long long c1 = (total + 3) >> 2, c2 = (total + 1) >> 1, c3 = (3 * total + 3) >> 2;
        unsigned long long C = 0;
        bool f1 = false, f2 = false, f3 = false;
        for (int k = 0; k < bins; ++k) {
            C += (unsigned long long)h[k];
            if (!f1 && C >= c1) { f1 = true; q1 = k; }
            if (!f2 && C >= c2) { f2 = true; m = k; }
            if (!f3 && C >= c3) { f3 = true; q3 = k; }
        }
        const int lo = m - a.trim < 0 ? 0 : m - a.trim, hi = m + a.trim > bins - 1 ? bins - 1 : m + a.trim;
        long long wsum = 0, msum = 0;
        for (int k = lo; k <= hi; ++k) { wsum += h[k]; msum += h[bins + k]; }
        lhat = a.L * ((double)msum / (double)wsum);                       // wsum >= W[m] > 0
        share = (double)wsum / (double)total;
    }
    for (int k = 0; k < PF_ODO_CELLS(bins); ++k) h[k] = 0;
    const double iqr = (double)(q3 - q1) * (2.0 * a.L) / (double)bins;
    const bool valid = sane && used >= (double)a.min_used && iqr <= (double)a.max_iqr && m != 0 && m != bins - 1;
    a.ratio[b] = valid ? (float)exp2(lhat) : 1.f;
    float* st = a.stats + (long)b * PF_ODO_STATS;
    st[0] = (float)sw; st[1] = (float)used; st[2] = (float)lhat; st[3] = (float)iqr; st[4] = (float)share; st[5] = valid ? 1.f : 0.f;
}

// ---- reverse pose ------------------------------------------------------------------------------------------------------------
PF_HD void pf_odo_reverse_image(const PfOdoReverseArgs& a, int b) {
    const float* R = a.R + (long)b * 9;
    const float* t = a.t + (long)b * 3;
    float* Rr = a.Rr + (long)b * 9;
    float* tr = a.tr + (long)b * 3;
    float m[9];
    for (int k = 0; k < 9; ++k) m[k] = R[k];
    const float t0 = t[0], t1 = t[1], t2 = t[2];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) Rr[i * 3 + j] = m[j * 3 + i];
        tr[i] = 0.f - ((m[i] * t0 + m[3 + i] * t1) + m[6 + i] * t2);
    }
}

// ---- track -------------------------------------------------------------------------------------------------------------------
PF_HD void pf_odo_track_image(const PfOdoTrackArgs& a, int i) {
    double* st = a.state + (long)i * PF_ODO_STATE;
    const float* R = a.R + (long)i * 9;
    const float* t = a.t + (long)i * 3;
    PfQuat A; A.a = st[0]; A.b = st[1]; A.c = st[2]; A.d = st[3];
    A = pf_quat_canon(pf_quat_mul(pf_quat_of(R), A));
    const double b0 = st[4], b1 = st[5], b2 = st[6];
    double b[3];
    for (int k = 0; k < 3; ++k) b[k] = ((double)R[k * 3] * b0 + (double)R[k * 3 + 1] * b1) + (double)R[k * 3 + 2] * b2;
    double S = st[7], steps = st[8], segment = st[9];
    const bool prev = st[10] != 0.0;
    const bool pv = a.pose_stats[(long)i * PF_EPI_STATS + 5] != 0.f, lv = a.link_stats[(long)i * PF_ODO_STATS + 5] != 0.f;
    if (pv) {
        if (prev && lv) S = S * (double)a.ratio[i]; else segment += 1.0;
        for (int k = 0; k < 3; ++k) b[k] = b[k] + S * (double)t[k];
    }
    steps += 1.0;
    st[0] = A.a; st[1] = A.b; st[2] = A.c; st[3] = A.d; st[4] = b[0]; st[5] = b[1]; st[6] = b[2];
    st[7] = S; st[8] = steps; st[9] = segment; st[10] = pv ? 1.0 : 0.0; st[11] = 0.0;
    float* O = a.orient + (long)i * 9;
    pf_quat_matrix(A, O);
    // centre = -A^T b with A's matrix in fp64
    const double aa = A.a * A.a, bb = A.b * A.b, cc = A.c * A.c, dd = A.d * A.d;
    const double M[9] = {aa + bb - cc - dd, 2.0 * (A.b * A.c - A.a * A.d), 2.0 * (A.b * A.d + A.a * A.c),
                         2.0 * (A.b * A.c + A.a * A.d), aa - bb + cc - dd, 2.0 * (A.c * A.d - A.a * A.b),
                         2.0 * (A.b * A.d - A.a * A.c), 2.0 * (A.c * A.d + A.a * A.b), aa - bb - cc + dd};
    for (int k = 0; k < 3; ++k) a.centre[(long)i * 3 + k] = (float)(0.0 - ((M[k] * b[0] + M[3 + k] * b[1]) + M[6 + k] * b[2]));
    a.baseline[i] = (float)S;
    int* fl = a.flags + (long)i * PF_ODO_FLAGS;
    fl[0] = (int)steps; fl[1] = (int)segment; fl[2] = pv ? 1 : 0; fl[3] = lv ? 1 : 0;
}

// ---- fuse --------------------------------------------------------------------------------------------------------------------
PF_HD bool pf_odo_counts(float k, float c, unsigned char m, float conf_min) { return m == 0 && c >= conf_min && k >= 0.f && k < PF_EGO_FAR; }
PF_HD void pf_odo_fuse_pixel(const PfOdoFuseArgs& a, int b, long n) {
    const long N = (long)a.H * a.W, o = (long)b * N + n;
    const float ka = a.a.inv[o], ca = a.a.conf[o], kb = a.b.inv[o], cb = a.b.conf[o];
    const bool oka = a.link_valid[b] != 0.f && pf_odo_counts(ka, ca, a.a.moving[o], a.conf_min);
    const bool okb = pf_odo_counts(kb, cb, a.b.moving[o], a.conf_min);
    const float wa = oka ? ca : 0.f, wb = okb ? cb : 0.f;
    const float da = oka ? ka / a.S_a[b] : 0.f, db = okb ? kb / a.S_b[b] : 0.f;
    const float ws = wa + wb;
    // a weight sum that is not positive and finite (conf = 0 under conf_min = 0, conf = inf) counts nothing: 0, never 0 / 0
    const bool some = (oka || okb) && ws > 0.f && pf_finite(ws);
    float inv = 0.f;
    if (some) inv = (wa * da + wb * db) / ws;
    unsigned char dis = 0;
    if (oka && okb && ka >= a.kappa_min && kb >= a.kappa_min) dis = fabsf(log2f(db / da)) > a.tol ? 1 : 0;
    if (a.inv_depth) a.inv_depth[o] = inv;
    if (a.weight) a.weight[o] = some ? ws : 0.f;
    if (a.disagree) a.disagree[o] = dis;
}

// ---- argument checks shared by the device entries and their host emulation ---------------------------------------------------
static inline bool pf_odo_meet(const void* p, long np, const void* q, long nq) {
    if (!p || !q) return false;
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + (uintptr_t)nq && b < a + (uintptr_t)np;
}
static inline bool pf_odo_bins_ok(int bins) { return bins >= 64 && bins <= 1024 && (bins & (bins - 1)) == 0; }
static inline long pf_odo_bytes(int B, int H, int W, int bins) {
    if (!pf_odo_bins_ok(bins)) return PF_ERR_BAD_ARG;
    const int rc = pf_ego_geometry(B, H, W);
    return rc != PF_OK ? rc : (long)B * PF_ODO_CELLS(bins) * 8;
}
static inline bool pf_odo_pos(float v) { return v > 0.f && pf_finite(v); }
static inline int pf_odo_accumulate_check(const float* inv_a, const float* conf_a, const unsigned char* moving_a, const float* inv_b,
                                          const float* conf_b, const unsigned char* moving_b, void* hist, int B, int H, int W, int bins,
                                          float log2_range, float kappa_min, int blocks, PfOdoAccArgs& a) {
    if (!inv_a || !conf_a || !moving_a || !inv_b || !conf_b || !moving_b || !hist || ((uintptr_t)hist & 7)) return PF_ERR_BAD_ARG;
    if (!pf_odo_bins_ok(bins) || !pf_odo_pos(log2_range) || !pf_odo_pos(kappa_min) || !(log2_range <= 64.f)) return PF_ERR_BAD_ARG;
    if (blocks < 0 || blocks > PF_EGO_MAX_GRID) return PF_ERR_BAD_ARG;
    const int rc = pf_ego_geometry(B, H, W);
    if (rc != PF_OK) return rc;
    const long N = (long)B * H * W, hb = (long)B * PF_ODO_CELLS(bins) * 8;
    const void* in[6] = {inv_a, conf_a, moving_a, inv_b, conf_b, moving_b};
    for (int i = 0; i < 6; ++i) if (pf_odo_meet(hist, hb, in[i], (i % 3 == 2) ? N : N * 4)) return PF_ERR_BAD_ARG;
    a.a.inv = inv_a; a.a.conf = conf_a; a.a.moving = moving_a; a.b.inv = inv_b; a.b.conf = conf_b; a.b.moving = moving_b;
    a.hist = static_cast<long long*>(hist); a.B = B; a.H = H; a.W = W; a.bins = bins;
    a.L = log2_range; a.two_L = 2.f * log2_range; a.binsf = (float)bins; a.kappa_min = kappa_min; a.f = pf_ego_scales(H, W).f;
    return PF_OK;
}
static inline int pf_odo_solve_check(void* hist, float* ratio, float* stats, int B, int H, int W, int bins, float log2_range,
                                     int trim_bins, float min_used, float max_iqr, PfOdoSolveArgs& a) {
    if (!hist || !ratio || !stats || ((uintptr_t)hist & 7)) return PF_ERR_BAD_ARG;
    if (!pf_odo_bins_ok(bins) || !pf_odo_pos(log2_range) || !(log2_range <= 64.f) || trim_bins < 0 || trim_bins > bins) return PF_ERR_BAD_ARG;
    if (!(min_used >= 0.f && pf_finite(min_used)) || !pf_odo_pos(max_iqr)) return PF_ERR_BAD_ARG;
    const int rc = pf_ego_geometry(B, H, W);
    if (rc != PF_OK) return rc;
    const long hb = (long)B * PF_ODO_CELLS(bins) * 8, rb = (long)B * 4, sb = (long)B * PF_ODO_STATS * 4;
    if (pf_odo_meet(hist, hb, ratio, rb) || pf_odo_meet(hist, hb, stats, sb) || pf_odo_meet(ratio, rb, stats, sb)) return PF_ERR_BAD_ARG;
    a.hist = static_cast<long long*>(hist); a.ratio = ratio; a.stats = stats; a.B = B; a.H = H; a.W = W; a.bins = bins;
    a.trim = trim_bins; a.min_used = min_used; a.max_iqr = max_iqr; a.L = (double)log2_range; a.inv = pf_ego_scales(H, W).inv;
    return PF_OK;
}
static inline int pf_odo_reverse_check(const float* R, const float* t, float* Rr, float* tr, int B, PfOdoReverseArgs& a) {
    if (!R || !t || !Rr || !tr) return PF_ERR_BAD_ARG;
    if (B < 1 || B > PF_EGO_MAX_GRID) return PF_ERR_BAD_SHAPE;
    const long mb = (long)B * 36, vb = (long)B * 12;
    if (pf_odo_meet(Rr, mb, R, mb) || pf_odo_meet(Rr, mb, t, vb) || pf_odo_meet(tr, vb, R, mb) || pf_odo_meet(tr, vb, t, vb)
        || pf_odo_meet(Rr, mb, tr, vb)) return PF_ERR_BAD_ARG;
    a.R = R; a.t = t; a.Rr = Rr; a.tr = tr; a.B = B;
    return PF_OK;
}
static inline int pf_odo_track_check(const float* R, const float* t, const float* pose_stats, const float* ratio, const float* link_stats,
                                     void* state, float* orient, float* centre, float* baseline, int* flags, int B, PfOdoTrackArgs& a) {
    if (!R || !t || !pose_stats || !ratio || !link_stats || !state || !orient || !centre || !baseline || !flags || ((uintptr_t)state & 7))
        return PF_ERR_BAD_ARG;
    if (B < 1 || B > PF_EGO_MAX_GRID) return PF_ERR_BAD_SHAPE;
    const void* in[5] = {R, t, pose_stats, ratio, link_stats};
    const long inb[5] = {(long)B * 36, (long)B * 12, (long)B * PF_EPI_STATS * 4, (long)B * 4, (long)B * PF_ODO_STATS * 4};
    const void* out[5] = {state, orient, centre, baseline, flags};
    const long outb[5] = {(long)B * PF_ODO_STATE * 8, (long)B * 36, (long)B * 12, (long)B * 4, (long)B * PF_ODO_FLAGS * 4};
    for (int i = 0; i < 5; ++i) {
        for (int j = 0; j < 5; ++j) if (pf_odo_meet(out[i], outb[i], in[j], inb[j])) return PF_ERR_BAD_ARG;
        for (int j = 0; j < i; ++j) if (pf_odo_meet(out[i], outb[i], out[j], outb[j])) return PF_ERR_BAD_ARG;
    }
    a.R = R; a.t = t; a.pose_stats = pose_stats; a.ratio = ratio; a.link_stats = link_stats; a.state = static_cast<double*>(state);
    a.orient = orient; a.centre = centre; a.baseline = baseline; a.flags = flags; a.B = B;
    return PF_OK;
}
static inline int pf_odo_fuse_check(const float* inv_a, const float* conf_a, const unsigned char* moving_a, const float* inv_b,
                                    const float* conf_b, const unsigned char* moving_b, const float* S_a, const float* S_b,
                                    const float* link_valid, float* inv_depth, float* weight, unsigned char* disagree, int B, int H, int W,
                                    float conf_min, float kappa_min, float tol_log2, PfOdoFuseArgs& a) {
    if (!inv_a || !conf_a || !moving_a || !inv_b || !conf_b || !moving_b || !S_a || !S_b || !link_valid) return PF_ERR_BAD_ARG;
    if (!(conf_min >= 0.f && pf_finite(conf_min)) || !pf_odo_pos(kappa_min) || !pf_odo_pos(tol_log2)) return PF_ERR_BAD_ARG;
    const int rc = pf_ego_geometry(B, H, W);
    if (rc != PF_OK) return rc;
    const long N = (long)B * H * W;
    const void* in[9] = {inv_a, conf_a, moving_a, inv_b, conf_b, moving_b, S_a, S_b, link_valid};
    const long inb[9] = {N * 4, N * 4, N, N * 4, N * 4, N, (long)B * 4, (long)B * 4, (long)B * 4};
    const void* out[3] = {inv_depth, weight, disagree};
    const long outb[3] = {N * 4, N * 4, N};
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 9; ++j) if (pf_odo_meet(out[i], outb[i], in[j], inb[j])) return PF_ERR_BAD_ARG;
        for (int j = 0; j < i; ++j) if (pf_odo_meet(out[i], outb[i], out[j], outb[j])) return PF_ERR_BAD_ARG;
    }
    a.a.inv = inv_a; a.a.conf = conf_a; a.a.moving = moving_a; a.b.inv = inv_b; a.b.conf = conf_b; a.b.moving = moving_b;
    a.S_a = S_a; a.S_b = S_b; a.link_valid = link_valid; a.inv_depth = inv_depth; a.weight = weight; a.disagree = disagree;
    a.B = B; a.H = H; a.W = W; a.conf_min = conf_min; a.kappa_min = kappa_min; a.tol = tol_log2;
    return PF_OK;
}
