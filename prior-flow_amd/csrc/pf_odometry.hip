// Camera trajectory from 360-degree video on the device: the per-pixel and per-image arithmetic is
// pf_odometry.h.  A link is two launches; nothing is read on the host.
//
//   pf_odo_acc_kernel         grid (blocks, B), blocks from the CU count, not from the image
//     pf_epi_acc_kernel's outer shape: 1024 threads; a wave takes kStrip * 64 consecutive pixels of ONE row at a time, so cos phi
//     is computed once per strip; the waves of the grid stride over the strips of the image.  The histogram of the workgroup
//     (2 bins 64-bit integers: 8 KB at 512 bins) lives in LDS and is filled with 64-bit LDS adds; the total and the count stay in
//     registers and are reduced like pf_epi_acc_kernel's sums.  At the end the workgroup makes one 64-bit global atomic, whose
//     result nobody reads, per non-zero cell.  Integer adds commute, so which way a contribution went does not change a bit.
//     A static scene puts nearly every pixel into one or two bins, 64 lanes on one LDS address.  Measured (DESIGN.md section
//     22), that input is no slower than one spread evenly over the bins (14.6 against 15.5 us at 512 x 1024), so every lane adds
//     alone; the form that combines inside the wave first, which gained 3 % on the one and lost 10 % on the other, is
//     profiles/odo_combine.hip.
//   pf_odo_solve_kernel       one lane per image: three passes over the cells (prefix sums, the window, the zeros)
//   pf_odo_reverse_kernel, pf_odo_track_kernel      one lane per image
//   pf_odo_fuse_kernel        one thread per pixel                                          grid (pixels / 256, B)
//
// Every access is at a pixel index below H * W, an image index below B or a cell index below 2 bins + 2; the bin of a pixel is
// clamped to 0..bins-1 after the tests that leave a pixel out (pf_odo_link_pixel), so no address depends on an input value.
#include "pf_odometry.h"

namespace {
constexpr int kBlock = 256;
constexpr int kAccBlock = 1024, kWaves = kAccBlock / 64;
constexpr int kStrip = 2;

__device__ inline long long wave_sum(long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}
__device__ inline void lds_add(unsigned long long* cell, long long v) { atomicAdd(cell, (unsigned long long)v); }

__global__ void __launch_bounds__(kAccBlock) pf_odo_acc_kernel(const PfOdoAccArgs a) {
    extern __shared__ unsigned long long hist[];                          // W[bins], M[bins]
    __shared__ long long part[kWaves][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y, bins = a.bins;
    const long N = (long)a.H * a.W;
    for (int c = tid; c < 2 * bins; c += kAccBlock) hist[c] = 0;
    __syncthreads();
    const float* ka = a.a.inv + (long)b * N;
    const float* ca = a.a.conf + (long)b * N;
    const unsigned char* ma = a.a.moving + (long)b * N;
    const float* kb = a.b.inv + (long)b * N;
    const float* cb = a.b.conf + (long)b * N;
    const unsigned char* mb = a.b.moving + (long)b * N;
    long long tot = 0, cnt = 0;
    const int per_row = (a.W + kStrip * 64 - 1) / (kStrip * 64);
    const long strips = (long)a.H * per_row;                            // < 2^30
    for (long i = (long)blockIdx.x * kWaves + wave; i < strips; i += (long)gridDim.x * kWaves) {
        const int y = (int)(i / per_row), xw = (int)(i - (long)y * per_row) * (kStrip * 64);
        float cp, sp;
        pf_ego_row(y, a.H, cp, sp);
        for (int k = 0; k < kStrip; ++k) {
            if (xw + k * 64 >= a.W) break;                              // the same for the whole wave
            const int x = xw + k * 64 + lane;
            int bin = 0;
            float w = 0.f, lc = 0.f;
            bool ok = false;
            if (x < a.W) {
                const long n = (long)y * a.W + x;
                ok = pf_odo_link_pixel(a, cp, ka[n], ca[n], ma[n], kb[n], cb[n], mb[n], bin, w, lc);
            }
            long long qw = 0, qm = 0;
            if (ok) { qw = pf_odo_qw(a, w); qm = pf_odo_qm(a, w, lc); }
            tot += qw;
            cnt += ok ? 1 : 0;
            if (ok) { lds_add(&hist[bin], qw); lds_add(&hist[bins + bin], qm); }
        }
    }
    tot = wave_sum(tot);
    cnt = wave_sum(cnt);
    if (lane == 0) { part[wave][0] = tot; part[wave][1] = cnt; }
    __syncthreads();
    unsigned long long* out = reinterpret_cast<unsigned long long*>(a.hist + (long)b * PF_ODO_CELLS(bins));
    for (int c = tid; c < 2 * bins; c += kAccBlock) {
        const unsigned long long v = hist[c];
        if (v != 0) atomicAdd(out + c, v);
    }
    if (tid < 2) {
        long long v = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) v += part[w][tid];
        if (v != 0) atomicAdd(out + 2 * bins + tid, (unsigned long long)v);
    }
}
__global__ void __launch_bounds__(64) pf_odo_solve_kernel(const PfOdoSolveArgs a) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b < a.B) pf_odo_solve_image(a, b);
}
__global__ void __launch_bounds__(64) pf_odo_reverse_kernel(const PfOdoReverseArgs a) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b < a.B) pf_odo_reverse_image(a, b);
}
__global__ void __launch_bounds__(64) pf_odo_track_kernel(const PfOdoTrackArgs a) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b < a.B) pf_odo_track_image(a, b);
}
__global__ void __launch_bounds__(kBlock) pf_odo_fuse_kernel(const PfOdoFuseArgs a) {
    const long pix = (long)blockIdx.x * kBlock + threadIdx.x;
    if (pix >= (long)a.H * a.W) return;
    pf_odo_fuse_pixel(a, (int)blockIdx.y, pix);
}
int pf_odo_cus() {
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

extern "C" long pf_odo_hist_bytes(int B, int H, int W, int bins) { return pf_odo_bytes(B, H, W, bins); }

extern "C" int pf_odo_accumulate(const float* inv_a, const float* conf_a, const unsigned char* moving_a, const float* inv_b,
                                 const float* conf_b, const unsigned char* moving_b, void* hist, int B, int H, int W, int bins,
                                 float log2_range, float kappa_min, int blocks, void* stream) {
    PfOdoAccArgs a;
    const int rc = pf_odo_accumulate_check(inv_a, conf_a, moving_a, inv_b, conf_b, moving_b, hist, B, H, W, bins, log2_range, kappa_min,
                                           blocks, a);
    if (rc != PF_OK) return rc;
    // one workgroup per CU over the whole batch, never more than there are strips
    const long strips = (long)H * ((W + kStrip * 64 - 1) / (kStrip * 64));
    long bx = blocks;
    if (bx == 0) {
        const long need = (strips + kWaves - 1) / kWaves, cap = pf_odo_cus() / B;
        bx = need < cap ? need : cap;
        if (bx < 1) bx = 1;
    }
    hipLaunchKernelGGL(pf_odo_acc_kernel, dim3((unsigned)bx, (unsigned)B), dim3(kAccBlock), (size_t)2 * bins * 8,
                       (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

extern "C" int pf_odo_solve(void* hist, float* ratio, float* stats, int B, int H, int W, int bins, float log2_range, int trim_bins,
                            float min_used, float max_iqr, void* stream) {
    PfOdoSolveArgs a;
    const int rc = pf_odo_solve_check(hist, ratio, stats, B, H, W, bins, log2_range, trim_bins, min_used, max_iqr, a);
    if (rc != PF_OK) return rc;
    hipLaunchKernelGGL(pf_odo_solve_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

extern "C" int pf_odo_reverse_pose(const float* R, const float* t, float* R_rev, float* t_rev, int B, void* stream) {
    PfOdoReverseArgs a;
    const int rc = pf_odo_reverse_check(R, t, R_rev, t_rev, B, a);
    if (rc != PF_OK) return rc;
    hipLaunchKernelGGL(pf_odo_reverse_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

extern "C" int pf_odo_track(const float* R, const float* t, const float* pose_stats, const float* ratio, const float* link_stats,
                            void* state, float* orient, float* centre, float* baseline, int* flags, int B, void* stream) {
    PfOdoTrackArgs a;
    const int rc = pf_odo_track_check(R, t, pose_stats, ratio, link_stats, state, orient, centre, baseline, flags, B, a);
    if (rc != PF_OK) return rc;
    hipLaunchKernelGGL(pf_odo_track_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

extern "C" int pf_odo_fuse(const float* inv_a, const float* conf_a, const unsigned char* moving_a, const float* inv_b, const float* conf_b,
                           const unsigned char* moving_b, const float* S_a, const float* S_b, const float* link_valid, float* inv_depth,
                           float* weight, unsigned char* disagree, int B, int H, int W, float conf_min, float kappa_min, float tol_log2,
                           void* stream) {
    PfOdoFuseArgs a;
    const int rc = pf_odo_fuse_check(inv_a, conf_a, moving_a, inv_b, conf_b, moving_b, S_a, S_b, link_valid, inv_depth, weight, disagree,
                                     B, H, W, conf_min, kappa_min, tol_log2, a);
    if (rc != PF_OK) return rc;
    hipLaunchKernelGGL(pf_odo_fuse_kernel, dim3((unsigned)(((long)H * W + kBlock - 1) / kBlock), (unsigned)B), dim3(kBlock), 0,
                       (hipStream_t)stream, a);
    return (int)hipGetLastError();
}
