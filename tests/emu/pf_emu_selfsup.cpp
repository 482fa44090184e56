// Host emulation of pf_selfsup_loss_batch -- TEST INFRASTRUCTURE ONLY (its own library, libpf_emu_selfsup.so).  The per-pixel
// arithmetic, the cut into chunks and the argument checks are prior-flow_amd/csrc/pf_selfsup.h, the file the device kernel
// compiles; the launch is restated as a loop over (image, chunk, pixel, term), a chunk's sums as sequential fp64 adds.  The product
// never loads this library.
//
// pf_emu_selfsup_order picks the order in which the pixels of a chunk are visited: 0 first to last, 1 reversed, any other value a
// fixed pseudo-random permutation seeded with it.  The gradients must not notice at all; the chunk sums only in the rounding of
// their fp64 adds (tests/test_selfsup_host.py).
#include <algorithm>
#include <numeric>
#include <vector>

#include "pf_selfsup.h"

static unsigned long long g_order = 0;
extern "C" void pf_emu_selfsup_order(unsigned long long seed) { g_order = seed; }

static std::vector<long> visit_order(long lo, long hi) {
    std::vector<long> order(hi > lo ? hi - lo : 0);
    std::iota(order.begin(), order.end(), lo);
    if (g_order == 1) std::reverse(order.begin(), order.end());
    else if (g_order > 1) {
        unsigned long long s = g_order;
        for (long i = (long)order.size() - 1; i > 0; --i) {            // Fisher-Yates on a 64-bit LCG
            s = s * 6364136223846793005ULL + 1442695040888963407ULL;
            std::swap(order[i], order[(long)((s >> 33) % (unsigned long long)(i + 1))]);
        }
    }
    return order;
}

extern "C" int pf_selfsup_loss_batch(const float* const* preds, const float* image1, const float* image2, const float* weight,
                                     const unsigned char* mask, const float* i_weights, float* const* grads, double* partials, int nblk,
                                     int n, int B, int H, int W, float w_photo, float w_smooth, float eps_photo, float eps_smooth,
                                     float edge_lambda, float max_flow, float z, int blocks, void*) {
    PfSelfSupArgs a;
    const int rc = pf_selfsup_check(preds, image1, image2, weight, mask, i_weights, grads, partials, nblk, n, B, H, W, w_photo, w_smooth,
                                    eps_photo, eps_smooth, edge_lambda, max_flow, z, blocks, a);
    if (rc != PF_OK) return rc;
    const long pixels = (long)H * W, chunk = pf_ss_chunk(H, W, nblk);
    for (long b = 0; b < B; ++b)
        for (int k = 0; k < nblk; ++k) {
            const long lo = k * chunk, hi = lo + chunk < pixels ? lo + chunk : pixels;
            std::vector<double> tot((size_t)n * PF_SS_SUMS, 0.0);
            for (long pix : visit_order(lo, hi)) {
                PfSsCtx c;
                pf_ss_context(a, b, pix, c);
                for (int i = 0; i < n; ++i) {
                    double s[PF_SS_SUMS] = {0.0, 0.0, 0.0, 0.0};
                    pf_ss_term(a, c, b, i, s);
                    for (int j = 0; j < PF_SS_SUMS; ++j) tot[(size_t)i * PF_SS_SUMS + j] += s[j];
                }
            }
            for (int i = 0; i < n; ++i)
                for (int j = 0; j < PF_SS_SUMS; ++j)
                    partials[(((long)i * B + b) * nblk + k) * PF_SS_SUMS + j] = tot[(size_t)i * PF_SS_SUMS + j];
        }
    return PF_OK;
}
extern "C" const char* pf_version(void) { return "priorflow self-supervised criterion host emulation (tests only)"; }
