// Camera rotation from 360-degree flow on the device: the per-pixel and per-image arithmetic is
// pf_egomotion.h.  A pass of an estimate is two launches, an estimate 2 * passes; nothing is read on the host.
//
//   pf_ego_acc_kernel       grid (blocks, B), blocks from the CU count, not from the image
//     1024 threads; a wave takes kStrip * 64 consecutive pixels of ONE row at a time (lane l the pixels l, l + 64, ...: whole
//     256-byte runs per load), so a thread's cos phi, sin phi are computed once per strip; the waves of the grid stride over the
//     strips of the image.  Sixteen waves to a workgroup put four on every SIMD (the chains of transcendentals hide each other's
//     latency) while the atomics stay twelve per workgroup.
//     The twelve 64-bit partial sums stay in registers, are reduced across the wave with cross-lane moves (two 32-bit halves per
//     sum), meet in LDS, and leave the workgroup as ONE 64-bit integer atomic per sum whose result nobody reads.  R_{k-1} is read
//     through a uniform address.  p and q are recomputed in every pass (six transcendentals per pixel) rather than q kept in a
//     scratch plane: measured both ways (profiles/ego_variants.hip, 512x1024), 14.3 + 3 * 14.2 = 56.9 us against
//     15.3 + 3 * 13.6 = 56.0 us with the plane, which costs 12 bytes per pixel and a second form of the kernel.  With 256-thread
//     workgroups (one wave per SIMD) a pass took 16.2 us.
//   pf_ego_solve_kernel     one lane per image: Horn's matrix, cyclic Jacobi in fp64, R and stats; zeroes the sums it read
//   pf_ego_track_kernel     one lane per image: orientation, virtual path, correction
//   pf_erp_rotate_kernel    one thread per output pixel                                  grid (pixels / 256, B)
//     (6.7 us at 512x1024, C = 3; two and four pixels of a row per thread, sharing the row's sin phi, cos phi: 7.9 and 8.0 us)
//   pf_ego_derot_kernel     one thread per pixel                                         grid (pixels / 256, B)
//
// Integer adds commute, so where and in which order an add is made does not change a bit of the sums.  Every read of a map goes
// through pf_wraptaps (indices inside the map for any bits) or a pixel index below H * W; nothing is indexed by a flow value.
#include "pf_egomotion.h"

namespace {
constexpr int kBlock = 256;
constexpr int kAccBlock = 1024, kWaves = kAccBlock / 64; // accumulate: sixteen waves share a workgroup's twelve atomics
constexpr int kStrip = 2;                                // pixels of a thread per strip: a wave's strip is 128 pixels of a row

__global__ void __launch_bounds__(kAccBlock) pf_ego_acc_kernel(const PfEgoAccArgs a) {
    __shared__ long long part[kWaves][PF_EGO_SUMS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y;
    const long N = (long)a.H * a.W;
    float R[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = a.R[b * 9 + k];                  // the same address in every lane
    const float* fu = a.flow + (long)b * 2 * N;
    const float* fv = fu + N;
    const unsigned char* mk = a.mask ? a.mask + (long)b * N : nullptr;
    long long s[PF_EGO_SUMS];
#pragma unroll
    for (int k = 0; k < PF_EGO_SUMS; ++k) s[k] = 0;
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
            pf_ego_pixel(a, R, cp, sp, y, x, fu[n], fv[n], mk ? mk[n] : (unsigned char)0, s);
        }
    }
#pragma unroll
    for (int k = 0; k < PF_EGO_SUMS; ++k) {
        long long v = s[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if (lane == 0) part[wave][k] = v;
    }
    __syncthreads();
    if (tid < PF_EGO_SUMS) {
        long long v = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) v += part[w][tid];
        if (v != 0) atomicAdd(reinterpret_cast<unsigned long long*>(a.sums + (long)b * PF_EGO_SUMS + tid), (unsigned long long)v);
    }
}
__global__ void __launch_bounds__(64) pf_ego_solve_kernel(const PfEgoSolveArgs a) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b < a.B) pf_ego_solve_image(a, b);
}
__global__ void __launch_bounds__(64) pf_ego_track_kernel(const PfEgoTrackArgs a) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b < a.B) pf_ego_track_image(a, b);
}
__global__ void __launch_bounds__(kBlock) pf_erp_rotate_kernel(const PfErpRotArgs a) {
    const int pix = blockIdx.x * kBlock + threadIdx.x, b = blockIdx.y;
    if (pix >= a.H * a.W) return;
    float R[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = a.R[b * 9 + k];
    const int y = pix / a.W;
    float cp, sp;
    pf_ego_row(y, a.H, cp, sp);
    pf_erp_rotate_pixel(a, R, b, y, pix - y * a.W, cp, sp);
}
__global__ void __launch_bounds__(kBlock) pf_ego_derot_kernel(const PfEgoDerotArgs a) {
    const int pix = blockIdx.x * kBlock + threadIdx.x, b = blockIdx.y;
    if (pix >= a.H * a.W) return;
    float R[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = a.R[b * 9 + k];
    const int y = pix / a.W;
    pf_ego_derotate_pixel(a, R, b, y, pix - y * a.W);
}
unsigned pf_ego_blocks(long items) { return (unsigned)((items + kBlock - 1) / kBlock); }
int pf_ego_cus() {
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

extern "C" long pf_ego_scratch_bytes(int B, int H, int W) { return pf_ego_bytes(B, H, W); }

extern "C" int pf_ego_accumulate(const float* flow, const unsigned char* mask, const float* R, void* sums, int B, int H, int W,
                                 int weighted, float scale_px, int blocks, void* stream) {
    PfEgoAccArgs a;
    const int rc = pf_ego_accumulate_check(flow, mask, R, sums, B, H, W, weighted, scale_px, blocks, a);
    if (rc != PF_OK) return rc;
    // one workgroup per CU over the whole batch, never more than there are strips: 12 atomics per workgroup
    const long strips = (long)H * ((W + kStrip * 64 - 1) / (kStrip * 64));
    long bx = blocks;
    if (bx == 0) {
        const long need = (strips + kWaves - 1) / kWaves, cap = pf_ego_cus() / B;
        bx = need < cap ? need : cap;
        if (bx < 1) bx = 1;
    }
    hipLaunchKernelGGL(pf_ego_acc_kernel, dim3((unsigned)bx, (unsigned)B), dim3(kAccBlock), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

extern "C" int pf_ego_solve(void* sums, const float* init, float* R, float* stats, int B, int H, int W, float gap_min, void* stream) {
    PfEgoSolveArgs a;
    const int rc = pf_ego_solve_check(sums, init, R, stats, B, H, W, gap_min, a);
    if (rc != PF_OK) return rc;
    hipLaunchKernelGGL(pf_ego_solve_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

extern "C" int pf_ego_track(const float* R, void* state, float* orient, float* corr, int B, float smoothing, void* stream) {
    PfEgoTrackArgs a;
    const int rc = pf_ego_track_check(R, state, orient, corr, B, smoothing, a);
    if (rc != PF_OK) return rc;
    hipLaunchKernelGGL(pf_ego_track_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

extern "C" int pf_erp_rotate(const void* in, void* out, const float* R, int B, int C, int H, int W, int form, void* stream) {
    PfErpRotArgs a;
    const int rc = pf_erp_rotate_check(in, out, R, B, C, H, W, form, a);
    if (rc != PF_OK) return rc;
    hipLaunchKernelGGL(pf_erp_rotate_kernel, dim3(pf_ego_blocks((long)H * W), (unsigned)B), dim3(kBlock), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

extern "C" int pf_ego_derotate(const float* flow, const unsigned char* mask, const float* R, float* out, unsigned char* valid, int B,
                               int H, int W, void* stream) {
    PfEgoDerotArgs a;
    const int rc = pf_ego_derotate_check(flow, mask, R, out, valid, B, H, W, a);
    if (rc != PF_OK) return rc;
    hipLaunchKernelGGL(pf_ego_derot_kernel, dim3(pf_ego_blocks((long)H * W), (unsigned)B), dim3(kBlock), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}
