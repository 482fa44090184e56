// Host emulation of pf_splat_accumulate / pf_splat_resolve -- TEST INFRASTRUCTURE ONLY (its own library, libpf_emu_splat.so).  The
// per-pixel arithmetic, the scales and the argument checks are prior-flow_amd/csrc/pf_splat.h, the file the device kernels compile;
// a launch is restated as a loop over its grid, an atomic add as a plain add.  The product never loads this library.
//
// pf_emu_splat_order picks the order in which the accumulate loop visits its (job, pixel) items: 0 as the grid counts them,
// 1 reversed, any other value a fixed pseudo-random permutation seeded with it.  Integer adds commute, so the sums must not
// notice (tests/test_splat_host.py).
#include <algorithm>
#include <numeric>
#include <vector>

#include "pf_splat.h"

static unsigned long long g_order = 0;
extern "C" void pf_emu_splat_order(unsigned long long seed) { g_order = seed; }

extern "C" long pf_splat_scratch_bytes(int B, int C, int H, int W) { return pf_splat_bytes(B, C, H, W); }

extern "C" int pf_splat_accumulate(const pf_splat_job* jobs, int njobs, void* acc, int B, int C, int H, int W, float alpha,
                                   float zmax, float vmax, void*) {
    PfSplatAccArgs a;
    const int rc = pf_splat_accumulate_check(jobs, njobs, acc, B, C, H, W, alpha, zmax, vmax, a);
    if (rc != PF_OK) return rc;
    const long N = (long)H * W, items = (long)njobs * B * N;
    std::vector<long> order(items);
    std::iota(order.begin(), order.end(), 0L);
    if (g_order == 1) std::reverse(order.begin(), order.end());
    else if (g_order > 1) {
        unsigned long long s = g_order;
        for (long i = items - 1; i > 0; --i) {                 // Fisher-Yates on a 64-bit LCG
            s = s * 6364136223846793005ULL + 1442695040888963407ULL;
            std::swap(order[i], order[(long)((s >> 33) % (unsigned long long)(i + 1))]);
        }
    }
    for (long it : order) {
        const int j = (int)(it / (B * N));
        const long r = it % (B * N), b = r / N, pix = r % N;
        const int y = (int)(pix / W);
        pf_splat_pixel(pf_splat_pick(a, j), a, b, y, (int)(pix - (long)y * W));
    }
    return PF_OK;
}

extern "C" int pf_splat_resolve(void* acc, float* out, unsigned char* hole, const float* fill0, const float* fill1, float fill_t,
                                float cmin, int njobs, int B, int C, int H, int W, float vmax, void*) {
    PfSplatResArgs a;
    const int rc = pf_splat_resolve_check(acc, out, hole, fill0, fill1, fill_t, cmin, njobs, B, C, H, W, vmax, a);
    if (rc != PF_OK) return rc;
    const long N = (long)H * W;
    const bool quads = pf_splat_quads(a);
    for (long b = 0; b < B; ++b) {
        if (quads) for (long n = 0; n < N; n += 4) pf_splat_resolve_quad(a, b, n);
        else for (long n = 0; n < N; ++n) pf_splat_resolve_pixel(a, b, n);
    }
    return PF_OK;
}

// the scales of a call, for the tests of the scale rule: out = {S_D, S_N}
extern "C" void pf_emu_splat_scales(int njobs, int H, int W, float vmax, int* out) {
    const PfSplatScales s = pf_splat_scales(njobs, H, W, vmax);
    out[0] = s.sd; out[1] = s.sn;
}
extern "C" const char* pf_version(void) { return "priorflow splat host emulation (tests only)"; }
