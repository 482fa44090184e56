// Host emulation of pf_epi_accumulate / pf_epi_solve / pf_epi_map, with the pf_ego_accumulate / pf_ego_solve a PoseEstimator's
// RotationEstimator needs -- TEST INFRASTRUCTURE ONLY (its own library, libpf_emu_epipolar.so).  The per-pixel and per-image
// arithmetic, the scales and the argument checks are prior-flow_amd/csrc/pf_epipolar.h and pf_egomotion.h, the files the device
// kernels compile; a launch is restated as a loop over its grid, an atomic add as a plain add.  The product never loads this
// library.
//
// pf_emu_epi_order picks the order in which the accumulate loops visit the pixels of an image: 0 row by row, 1 reversed, any
// other value a fixed pseudo-random permutation seeded with it.  Integer adds commute, so the sums must not notice
// (tests/test_epipolar_host.py).
#include <algorithm>
#include <numeric>
#include <vector>

#include "pf_epipolar.h"

static unsigned long long g_order = 0;
extern "C" void pf_emu_epi_order(unsigned long long seed) { g_order = seed; }

static std::vector<long> visit_order(long N) {
    std::vector<long> order(N);
    std::iota(order.begin(), order.end(), 0L);
    if (g_order == 1) std::reverse(order.begin(), order.end());
    else if (g_order > 1) {
        unsigned long long s = g_order;
        for (long i = N - 1; i > 0; --i) {                     // Fisher-Yates on a 64-bit LCG
            s = s * 6364136223846793005ULL + 1442695040888963407ULL;
            std::swap(order[i], order[(long)((s >> 33) % (unsigned long long)(i + 1))]);
        }
    }
    return order;
}

extern "C" long pf_ego_scratch_bytes(int B, int H, int W) { return pf_ego_bytes(B, H, W); }
extern "C" long pf_epi_sums_bytes(int B, int H, int W) { return pf_epi_bytes(B, H, W); }

extern "C" int pf_ego_accumulate(const float* flow, const unsigned char* mask, const float* R, void* sums, int B, int H, int W,
                                 int weighted, float scale_px, int blocks, void*) {
    PfEgoAccArgs a;
    const int rc = pf_ego_accumulate_check(flow, mask, R, sums, B, H, W, weighted, scale_px, blocks, a);
    if (rc != PF_OK) return rc;
    const long N = (long)H * W;
    const std::vector<long> order = visit_order(N);
    for (long b = 0; b < B; ++b) {
        const float* fu = flow + b * 2 * N;
        const float* fv = fu + N;
        for (long n : order) {
            const int y = (int)(n / W), x = (int)(n - (long)y * W);
            float cp, sp;
            pf_ego_row(y, H, cp, sp);
            pf_ego_pixel(a, R + b * 9, cp, sp, y, x, fu[n], fv[n], mask ? mask[b * N + n] : (unsigned char)0, a.sums + b * PF_EGO_SUMS);
        }
    }
    return PF_OK;
}

extern "C" int pf_ego_solve(void* sums, const float* init, float* R, float* stats, int B, int H, int W, float gap_min, void*) {
    PfEgoSolveArgs a;
    const int rc = pf_ego_solve_check(sums, init, R, stats, B, H, W, gap_min, a);
    if (rc != PF_OK) return rc;
    for (int b = 0; b < B; ++b) pf_ego_solve_image(a, b);
    return PF_OK;
}

extern "C" int pf_epi_accumulate(const float* flow, const unsigned char* mask, const float* R, const float* t, void* sums, int B, int H,
                                 int W, int mode, float scale_px, float vote_px, int blocks, void*) {
    PfEpiAccArgs a;
    const int rc = pf_epi_accumulate_check(flow, mask, R, t, sums, B, H, W, mode, scale_px, vote_px, blocks, a);
    if (rc != PF_OK) return rc;
    const long N = (long)H * W;
    const std::vector<long> order = visit_order(N);
    for (long b = 0; b < B; ++b) {
        const float* fu = flow + b * 2 * N;
        const float* fv = fu + N;
        PfVec3 tb;
        tb.x = t ? t[b * 3] : 0.f; tb.y = t ? t[b * 3 + 1] : 0.f; tb.z = t ? t[b * 3 + 2] : 0.f;
        for (long n : order) {
            const int y = (int)(n / W), x = (int)(n - (long)y * W);
            float cp, sp;
            pf_ego_row(y, H, cp, sp);
            const unsigned char m = mask ? mask[b * N + n] : (unsigned char)0;
            if (mode == PF_EPI_T) pf_epi_pixel<PF_EPI_T>(a, R + b * 9, tb, cp, sp, y, x, fu[n], fv[n], m, a.sums + b * PF_EPI_SUMS);
            else pf_epi_pixel<PF_EPI_R>(a, R + b * 9, tb, cp, sp, y, x, fu[n], fv[n], m, a.sums + b * PF_EPI_SUMS);
        }
    }
    return PF_OK;
}

extern "C" int pf_epi_solve(void* sums, const float* t_init, float* R, float* t, float* stats, int B, int H, int W, int mode,
                            float gap_min, float min_parallax_px, void*) {
    PfEpiSolveArgs a;
    const int rc = pf_epi_solve_check(sums, t_init, R, t, stats, B, H, W, mode, gap_min, min_parallax_px, a);
    if (rc != PF_OK) return rc;
    for (int b = 0; b < B; ++b) pf_epi_solve_image(a, b);
    return PF_OK;
}

extern "C" int pf_epi_map(const float* flow, const unsigned char* mask, const float* R, const float* t, float* inv_depth, float* resid,
                          float* conf, unsigned char* moving, int B, int H, int W, float thr_px, float neg_px, float conf_min, void*) {
    PfEpiMapArgs a;
    const int rc = pf_epi_map_check(flow, mask, R, t, inv_depth, resid, conf, moving, B, H, W, thr_px, neg_px, conf_min, a);
    if (rc != PF_OK) return rc;
    for (int b = 0; b < B; ++b) {
        PfVec3 tb;
        tb.x = t[b * 3]; tb.y = t[b * 3 + 1]; tb.z = t[b * 3 + 2];
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) pf_epi_map_pixel(a, R + (long)b * 9, tb, b, y, x);
    }
    return PF_OK;
}

// the worst-case row of the overflow argument: n pixels that each add the largest contribution of a sum bounded by 1 (at 2^S) and
// of one bounded by 4 (at 2^(S-2)), through pf_ego_quant; out = {the sum at S, the sum at S - 2}
extern "C" void pf_emu_epi_worst(int H, int W, long long* out) {
    const PfEgoScales s = pf_ego_scales(H, W);
    long long a = 0, b = 0;
    for (long i = 0; i < (long)H * W; ++i) { a += pf_ego_quant(1.f, s.f); b += pf_ego_quant(4.f, s.fr); }
    out[0] = a; out[1] = b;
}
extern "C" const char* pf_version(void) { return "priorflow epipolar host emulation (tests only)"; }
