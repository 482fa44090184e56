// Host emulation of pf_ego_accumulate / pf_ego_solve / pf_ego_track / pf_erp_rotate / pf_ego_derotate -- TEST INFRASTRUCTURE ONLY
// (its own library, libpf_emu_egomotion.so).  The per-pixel and per-image arithmetic, the scales and the argument checks are
// prior-flow_amd/csrc/pf_egomotion.h, the file the device kernels compile; a launch is restated as a loop over its grid, an atomic
// add as a plain add.  The product never loads this library.
//
// pf_emu_ego_order picks the order in which the accumulate loop visits the pixels of an image: 0 row by row, 1 reversed, any
// other value a fixed pseudo-random permutation seeded with it.  Integer adds commute, so the sums must not notice
// (tests/test_egomotion_host.py).
#include <algorithm>
#include <numeric>
#include <vector>

#include "pf_egomotion.h"

static unsigned long long g_order = 0;
extern "C" void pf_emu_ego_order(unsigned long long seed) { g_order = seed; }

extern "C" long pf_ego_scratch_bytes(int B, int H, int W) { return pf_ego_bytes(B, H, W); }

extern "C" int pf_ego_accumulate(const float* flow, const unsigned char* mask, const float* R, void* sums, int B, int H, int W,
                                 int weighted, float scale_px, int blocks, void*) {
    PfEgoAccArgs a;
    const int rc = pf_ego_accumulate_check(flow, mask, R, sums, B, H, W, weighted, scale_px, blocks, a);
    if (rc != PF_OK) return rc;
    const long N = (long)H * W;
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

extern "C" int pf_ego_track(const float* R, void* state, float* orient, float* corr, int B, float smoothing, void*) {
    PfEgoTrackArgs a;
    const int rc = pf_ego_track_check(R, state, orient, corr, B, smoothing, a);
    if (rc != PF_OK) return rc;
    for (int b = 0; b < B; ++b) pf_ego_track_image(a, b);
    return PF_OK;
}

extern "C" int pf_erp_rotate(const void* in, void* out, const float* R, int B, int C, int H, int W, int form, void*) {
    PfErpRotArgs a;
    const int rc = pf_erp_rotate_check(in, out, R, B, C, H, W, form, a);
    if (rc != PF_OK) return rc;
    for (int b = 0; b < B; ++b)
        for (int y = 0; y < H; ++y) {
            float cp, sp;
            pf_ego_row(y, H, cp, sp);
            for (int x = 0; x < W; ++x) pf_erp_rotate_pixel(a, R + (long)b * 9, b, y, x, cp, sp);
        }
    return PF_OK;
}

extern "C" int pf_ego_derotate(const float* flow, const unsigned char* mask, const float* R, float* out, unsigned char* valid, int B,
                               int H, int W, void*) {
    PfEgoDerotArgs a;
    const int rc = pf_ego_derotate_check(flow, mask, R, out, valid, B, H, W, a);
    if (rc != PF_OK) return rc;
    for (int b = 0; b < B; ++b)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) pf_ego_derotate_pixel(a, R + (long)b * 9, b, y, x);
    return PF_OK;
}

// the scales of a geometry, for the tests of the scale rule: out = {S, S_r}
extern "C" void pf_emu_ego_scales(int H, int W, int* out) {
    const PfEgoScales s = pf_ego_scales(H, W);
    out[0] = s.s; out[1] = s.sr;
}
extern "C" const char* pf_version(void) { return "priorflow egomotion host emulation (tests only)"; }
