// Self-supervised criterion on the device: the arithmetic is pf_selfsup.h.  ONE launch covers the n <= 32
// predictions of a branch.
//
//   pf_selfsup_kernel   256 threads; a workgroup takes (chunk, image) items, blockIdx.x, blockIdx.x + gridDim.x, ...
//     A thread owns one pixel at a time, so the lanes of a wave read consecutive floats of a row.  It builds the pixel's
//     context ONCE (image1 at the pixel and its four neighbours, weight / Z, mask, and the four pair coefficients
//     with their expf) and keeps it in registers while it walks the n predictions: per prediction the flow of the pixel and of
//     its four neighbours, twelve tap values, two gradient stores; no branch stands around a load.  The four sums of a
//     prediction are reduced across the wave in fp64 with __shfl_down and added by lane 0 to the wave's own LDS cell (32 terms x
//     4 waves x 4 sums x 8 B = 4 KB; no other wave touches it).  When the chunk's pixels are done the four waves' cells are added
//     in wave order and stored: one fp64 store per (term, chunk, sum).
//
// Which pixels belong to a chunk is fixed by nblk (pf_ss_chunk), and which thread of a workgroup takes which pixel by the pixel's
// place in its chunk, so the grid changes neither the gradient bits nor the partials.  All stores are ordinary vector stores.  Every
// access is at a pixel index below H * W of an image index below B (pf_selfsup.h).
#include "pf_selfsup.h"

namespace {
constexpr int kBlock = 256, kWaves = kBlock / 64;

__global__ void __launch_bounds__(kBlock) pf_selfsup_kernel(const PfSelfSupArgs a) {
    __shared__ double cell[PF_SS_MAX][kWaves][PF_SS_SUMS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long pixels = (long)a.H * a.W, chunk = pf_ss_chunk(a.H, a.W, a.nblk);
    const long items = (long)a.nblk * a.B;
    for (long item = blockIdx.x; item < items; item += gridDim.x) {
        const long b = item / a.nblk;
        const int k = (int)(item - b * a.nblk);
        const long lo = k * chunk, hi = lo + chunk < pixels ? lo + chunk : pixels;
        for (int i = tid; i < PF_SS_MAX * kWaves * PF_SS_SUMS; i += kBlock) (&cell[0][0][0])[i] = 0.0;
        __syncthreads();
        for (long base = lo; base < hi; base += kBlock) {                 // uniform trip count: the shuffles see whole waves
            const long pix = base + tid;
            const bool live = pix < hi;
            PfSsCtx c;
            if (live) pf_ss_context(a, b, pix, c);
            for (int i = 0; i < a.n; ++i) {
                double s[PF_SS_SUMS] = {0.0, 0.0, 0.0, 0.0};
                if (live) pf_ss_term(a, c, b, i, s);
#pragma unroll
                for (int j = 0; j < PF_SS_SUMS; ++j) {
                    double v = s[j];
#pragma unroll
                    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
                    if (lane == 0) cell[i][wave][j] += v;
                }
            }
        }
        __syncthreads();
        for (int i = tid; i < a.n * PF_SS_SUMS; i += kBlock) {
            const int term = i / PF_SS_SUMS, j = i - term * PF_SS_SUMS;
            a.partials[(((long)term * a.B + b) * a.nblk + k) * PF_SS_SUMS + j] =
                ((cell[term][0][j] + cell[term][1][j]) + cell[term][2][j]) + cell[term][3][j];
        }
        __syncthreads();
    }
}
}  // namespace

extern "C" int pf_selfsup_loss_batch(const float* const* preds, const float* image1, const float* image2, const float* weight,
                                     const unsigned char* mask, const float* i_weights, float* const* grads, double* partials, int nblk,
                                     int n, int B, int H, int W, float w_photo, float w_smooth, float eps_photo, float eps_smooth,
                                     float edge_lambda, float max_flow, float z, int blocks, void* stream) {
    PfSelfSupArgs a;
    const int rc = pf_selfsup_check(preds, image1, image2, weight, mask, i_weights, grads, partials, nblk, n, B, H, W, w_photo, w_smooth,
                                    eps_photo, eps_smooth, edge_lambda, max_flow, z, blocks, a);
    if (rc != PF_OK) return rc;
    const long items = (long)nblk * B;                                    // <= 4096 * B
    long grid = blocks > 0 ? blocks : items;
    if (grid > items) grid = items;
    if (grid > PF_SS_MAX_GRID) grid = PF_SS_MAX_GRID;
    hipLaunchKernelGGL(pf_selfsup_kernel, dim3((unsigned)grid), dim3(kBlock), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}
