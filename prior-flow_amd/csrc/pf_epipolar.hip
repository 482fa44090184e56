// Camera translation from 360-degree flow on the device: the per-pixel and per-image arithmetic is
// pf_epipolar.h.  A pass of an estimate is two launches; nothing is read on the host.
//
//   pf_epi_acc_kernel<MODE>   grid (blocks, B), blocks from the CU count, not from the image
//     pf_ego_acc_kernel's shape: 1024 threads; a wave takes kStrip * 64 consecutive pixels of ONE row at a time (whole 256-byte
//     runs per load), so cos phi, sin phi are computed once per strip; the waves of the grid stride over the strips of the image.
//     The partial sums of the mode (13 for a T pass, 11 for an R pass) stay in registers as 64-bit integers, are reduced across
//     the wave with cross-lane moves (two 32-bit halves per sum), meet in LDS (16 waves x 22 x 8 B = 2.8 KB), and leave the
//     workgroup as ONE 64-bit integer atomic per non-zero sum whose result nobody reads.  R and t are read through uniform
//     addresses.  Per pixel: the six transcendentals of p and q as in pf_ego_acc_kernel, plus one division and two square roots
//     (the residual's |m| and the vote's normalisation) in a T pass, one of each in an R pass.
//   pf_epi_solve_kernel       one lane per image: 3 x 3 cyclic Jacobi in fp64; t and stats, or R in place; zeroes the sums it read
//   pf_epi_map_kernel         one thread per pixel                                          grid (pixels / 256, B)
//
// Integer adds commute, so where and in which order an add is made does not change a bit of the sums.  Every access is at a
// pixel index below H * W or an image index below B; nothing is indexed by a flow value.
#include "pf_epipolar.h"

namespace {
constexpr int kBlock = 256;
constexpr int kAccBlock = 1024, kWaves = kAccBlock / 64;
constexpr int kStrip = 2;

// the sums a pass of MODE adds to (pf_epipolar.h)
template <int MODE> __device__ constexpr bool in_mode(int k) { return MODE == PF_EPI_T ? k <= 12 : (k == 9 || k >= 12); }

template <int MODE>
__global__ void __launch_bounds__(kAccBlock) pf_epi_acc_kernel(const PfEpiAccArgs a) {
    __shared__ long long part[kWaves][PF_EPI_SUMS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y;
    const long N = (long)a.H * a.W;
    float R[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = a.R[b * 9 + k];                  // the same address in every lane
    PfVec3 t;
    t.x = a.t ? a.t[b * 3] : 0.f; t.y = a.t ? a.t[b * 3 + 1] : 0.f; t.z = a.t ? a.t[b * 3 + 2] : 0.f;
    const float* fu = a.flow + (long)b * 2 * N;
    const float* fv = fu + N;
    const unsigned char* mk = a.mask ? a.mask + (long)b * N : nullptr;
    long long s[PF_EPI_SUMS];
#pragma unroll
    for (int k = 0; k < PF_EPI_SUMS; ++k) s[k] = 0;
    const int per_row = (a.W + kStrip * 64 - 1) / (kStrip * 64);
    const long strips = (long)a.H * per_row;                            // < 2^30
    for (long i = (long)blockIdx.x * kWaves + wave; i < strips; i += (long)gridDim.x * kWaves) {
        const int y = (int)(i / per_row), x0 = (int)(i - (long)y * per_row) * (kStrip * 64) + lane;
        float cp, sp;
        pf_ego_row(y, a.H, cp, sp);
        for (int k = 0; k < kStrip; ++k) {
            const int x = x0 + k * 64;
            if (x >= a.W) break;
            const long n = (long)y * a.W + x;
            pf_epi_pixel<MODE>(a, R, t, cp, sp, y, x, fu[n], fv[n], mk ? mk[n] : (unsigned char)0, s);
        }
    }
#pragma unroll
    for (int k = 0; k < PF_EPI_SUMS; ++k) {
        if (!in_mode<MODE>(k)) continue;
        long long v = s[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if (lane == 0) part[wave][k] = v;
    }
    __syncthreads();
    if (tid < PF_EPI_SUMS && in_mode<MODE>(tid)) {
        long long v = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) v += part[w][tid];
        if (v != 0) atomicAdd(reinterpret_cast<unsigned long long*>(a.sums + (long)b * PF_EPI_SUMS + tid), (unsigned long long)v);
    }
}
__global__ void __launch_bounds__(64) pf_epi_solve_kernel(const PfEpiSolveArgs a) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b < a.B) pf_epi_solve_image(a, b);
}
__global__ void __launch_bounds__(kBlock) pf_epi_map_kernel(const PfEpiMapArgs a) {
    const int pix = blockIdx.x * kBlock + threadIdx.x, b = blockIdx.y;
    if (pix >= a.H * a.W) return;
    float R[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = a.R[b * 9 + k];
    PfVec3 t;
    t.x = a.t[b * 3]; t.y = a.t[b * 3 + 1]; t.z = a.t[b * 3 + 2];
    const int y = pix / a.W;
    pf_epi_map_pixel(a, R, t, b, y, pix - y * a.W);
}
int pf_epi_cus() {
    constexpr int MAX_DEV = 64;
    static int cus_of[MAX_DEV] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEV) dev = 0;
    if (cus_of[dev] == 0) {
        int n = 256;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cus_of[dev] = n;
    }
    return cus_of[dev];
}
}  // namespace

extern "C" long pf_epi_sums_bytes(int B, int H, int W) { return pf_epi_bytes(B, H, W); }

extern "C" int pf_epi_accumulate(const float* flow, const unsigned char* mask, const float* R, const float* t, void* sums, int B, int H,
                                 int W, int mode, float scale_px, float vote_px, int blocks, void* stream) {
    PfEpiAccArgs a;
    const int rc = pf_epi_accumulate_check(flow, mask, R, t, sums, B, H, W, mode, scale_px, vote_px, blocks, a);
    if (rc != PF_OK) return rc;
    // one workgroup per CU over the whole batch, never more than there are strips
    const long strips = (long)H * ((W + kStrip * 64 - 1) / (kStrip * 64));
    long bx = blocks;
    if (bx == 0) {
        const long need = (strips + kWaves - 1) / kWaves, cap = pf_epi_cus() / B;
        bx = need < cap ? need : cap;
        if (bx < 1) bx = 1;
    }
    const dim3 grid((unsigned)bx, (unsigned)B);
    if (mode == PF_EPI_T) hipLaunchKernelGGL(pf_epi_acc_kernel<PF_EPI_T>, grid, dim3(kAccBlock), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(pf_epi_acc_kernel<PF_EPI_R>, grid, dim3(kAccBlock), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

extern "C" int pf_epi_solve(void* sums, const float* t_init, float* R, float* t, float* stats, int B, int H, int W, int mode,
                            float gap_min, float min_parallax_px, void* stream) {
    PfEpiSolveArgs a;
    const int rc = pf_epi_solve_check(sums, t_init, R, t, stats, B, H, W, mode, gap_min, min_parallax_px, a);
    if (rc != PF_OK) return rc;
    hipLaunchKernelGGL(pf_epi_solve_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

extern "C" int pf_epi_map(const float* flow, const unsigned char* mask, const float* R, const float* t, float* inv_depth, float* resid,
                          float* conf, unsigned char* moving, int B, int H, int W, float thr_px, float neg_px, float conf_min,
                          void* stream) {
    PfEpiMapArgs a;
    const int rc = pf_epi_map_check(flow, mask, R, t, inv_depth, resid, conf, moving, B, H, W, thr_px, neg_px, conf_min, a);
    if (rc != PF_OK) return rc;
    hipLaunchKernelGGL(pf_epi_map_kernel, dim3((unsigned)(((long)H * W + kBlock - 1) / kBlock), (unsigned)B), dim3(kBlock), 0,
                       (hipStream_t)stream, a);
    return (int)hipGetLastError();
}
