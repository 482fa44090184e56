// Depth along the trajectory on the device: the per-pixel arithmetic is pf_reproject.h.  Everything runs on
// the stream it is given, reads nothing on the host and allocates nothing.
//
//   pf_reproj_kernel        grid (strips / 4, B), 256 threads
//     section 20's strip shape without the reduction: a wave takes kStrip * 64 consecutive pixels of ONE row (whole 256-byte runs
//     per load), so cos phi, sin phi are computed once per strip; R and T of the image are read through uniform addresses and
//     live in scalar registers.  Per pixel two transcendentals for p, two atan2f and two square roots for the landing point.
//   pf_zs_front_kernel      one thread per SOURCE pixel                                  grid (pixels / 256, B)
//     up to four 32-bit atomic maxima whose result nobody reads
//   pf_zs_acc_kernel        one thread per SOURCE pixel                                  grid (pixels / 256, B)
//     the same taps; per counting tap one 4-byte load of front and C + 3 64-bit integer atomics whose result nobody reads
//   pf_zs_res_kernel / pf_zs_res4_kernel      one thread per TARGET pixel, or per four of them (16-byte loads and stores) where
//     W % 4 == 0 and the maps are aligned, as pf_splat_resolve decides it
//   pf_du_kernel / pf_du4_kernel              one thread per pixel, or per four where H W % 4 == 0 and the maps are aligned;
//   pf_du_seg_kernel                          one thread per image, AFTER the pixel pass on the same stream
//
// Every index is a pixel index below H * W or an image index below B, except the taps of the splat: their column is wrapped into
// [0, W) and their row tested against [0, H) after the test that the landing point is finite and nearer than 2^30
// (pf_zsplat_taps), so no kernel can touch memory outside its maps whatever the inputs hold.
#include "pf_reproject.h"

namespace {
constexpr int kBlock = 256, kWaves = kBlock / 64;
constexpr int kStrip = 2;

__global__ void __launch_bounds__(kBlock) pf_reproj_kernel(const PfReprojArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.y;
    const int per_row = (a.W + kStrip * 64 - 1) / (kStrip * 64);
    const long strips = (long)a.H * per_row, i = (long)blockIdx.x * kWaves + wave;
    if (i >= strips) return;
    float R[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = a.R[b * 9 + k];                  // the same address in every lane
    PfVec3 T;
    T.x = a.T[b * 3]; T.y = a.T[b * 3 + 1]; T.z = a.T[b * 3 + 2];
    const int y = (int)(i / per_row), x0 = (int)(i - (long)y * per_row) * (kStrip * 64) + lane;
    float cp, sp;
    pf_ego_row(y, a.H, cp, sp);
#pragma unroll
    for (int k = 0; k < kStrip; ++k) {
        const int x = x0 + k * 64;
        if (x < a.W) pf_reproj_pixel(a, R, T, b, y, x, cp, sp);
    }
}
__global__ void __launch_bounds__(kBlock) pf_zs_front_kernel(const PfZsplatArgs a) {
    const int pix = blockIdx.x * kBlock + threadIdx.x;
    if (pix >= a.H * a.W) return;
    const int y = pix / a.W;
    pf_zsplat_front_pixel(a, (long)blockIdx.y, y, pix - y * a.W);
}
__global__ void __launch_bounds__(kBlock) pf_zs_acc_kernel(const PfZsplatArgs a) {
    const int pix = blockIdx.x * kBlock + threadIdx.x;
    if (pix >= a.H * a.W) return;
    const int y = pix / a.W;
    pf_zsplat_acc_pixel(a, (long)blockIdx.y, y, pix - y * a.W);
}
__global__ void __launch_bounds__(kBlock) pf_zs_res_kernel(const PfZsplatResArgs a) {
    const int pix = blockIdx.x * kBlock + threadIdx.x;
    if (pix < a.H * a.W) pf_zsplat_resolve_pixel(a, (long)blockIdx.y, pix);
}
__global__ void __launch_bounds__(kBlock) pf_zs_res4_kernel(const PfZsplatResArgs a) {
    const int quad = blockIdx.x * kBlock + threadIdx.x;
    if (quad < a.H * a.W / 4) pf_zsplat_resolve_quad(a, (long)blockIdx.y, 4L * quad);
}
__global__ void __launch_bounds__(kBlock) pf_du_kernel(const PfDepthUpdArgs a) {
    const int pix = blockIdx.x * kBlock + threadIdx.x;
    if (pix < a.H * a.W) pf_depth_update_pixel(a, (long)blockIdx.y, pix);
}
__global__ void __launch_bounds__(kBlock) pf_du4_kernel(const PfDepthUpdArgs a) {
    const int quad = blockIdx.x * kBlock + threadIdx.x;
    if (quad < a.H * a.W / 4) pf_depth_update_quad(a, (long)blockIdx.y, 4L * quad);
}
__global__ void __launch_bounds__(64) pf_du_seg_kernel(const PfDepthUpdArgs a) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b < a.B) pf_depth_seg_image(a, b);
}
unsigned pf_rp_blocks(long items) { return (unsigned)((items + kBlock - 1) / kBlock); }
}  // namespace

extern "C" int pf_reproj_project(const float* inv_depth, const float* weight, const unsigned char* mask, const float* R, const float* T,
                                 float* flow, float* d_new, unsigned char* valid, int B, int H, int W, float n_min, void* stream) {
    PfReprojArgs a;
    const int rc = pf_reproj_project_check(inv_depth, weight, mask, R, T, flow, d_new, valid, B, H, W, n_min, a);
    if (rc != PF_OK) return rc;
    const long strips = (long)H * ((W + kStrip * 64 - 1) / (kStrip * 64));                    // < 2^30 / 128 + H
    hipLaunchKernelGGL(pf_reproj_kernel, dim3((unsigned)((strips + kWaves - 1) / kWaves), (unsigned)B), dim3(kBlock), 0,
                       (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

extern "C" long pf_zsplat_bytes(int B, int C, int H, int W) { return pf_zsplat_acc_bytes(B, C, H, W); }

extern "C" int pf_zsplat_front(const float* src, const float* flow, const float* d, const float* weight, const unsigned char* valid,
                               void* front, int B, int C, int H, int W, float b_min, void* stream) {
    PfZsplatArgs a;
    const int rc = pf_zsplat_check(src, flow, d, weight, valid, front, nullptr, false, B, C, H, W, b_min, 0.f, 1.f, 1.f, 1.f, a);
    if (rc != PF_OK) return rc;
    hipLaunchKernelGGL(pf_zs_front_kernel, dim3(pf_rp_blocks((long)H * W), (unsigned)B), dim3(kBlock), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

extern "C" int pf_zsplat_accumulate(const float* src, const float* flow, const float* d, const float* weight, const unsigned char* valid,
                                    const void* front, void* acc, int B, int C, int H, int W, float b_min, float tol_log2, float w_max,
                                    float dmax, float vmax, void* stream) {
    PfZsplatArgs a;
    const int rc = pf_zsplat_check(src, flow, d, weight, valid, const_cast<void*>(front), acc, true, B, C, H, W, b_min, tol_log2, w_max,
                                   dmax, vmax, a);
    if (rc != PF_OK) return rc;
    hipLaunchKernelGGL(pf_zs_acc_kernel, dim3(pf_rp_blocks((long)H * W), (unsigned)B), dim3(kBlock), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

extern "C" int pf_zsplat_resolve(void* acc, void* front, float* out, float* d_out, float* w_out, unsigned char* hole, int B, int C, int H,
                                 int W, float cmin, float w_max, float dmax, float vmax, void* stream) {
    PfZsplatResArgs a;
    const int rc = pf_zsplat_resolve_check(acc, front, out, d_out, w_out, hole, B, C, H, W, cmin, w_max, dmax, vmax, a);
    if (rc != PF_OK) return rc;
    if (pf_zsplat_quads(a))
        hipLaunchKernelGGL(pf_zs_res4_kernel, dim3(pf_rp_blocks((long)H * W / 4), (unsigned)B), dim3(kBlock), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(pf_zs_res_kernel, dim3(pf_rp_blocks((long)H * W), (unsigned)B), dim3(kBlock), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

extern "C" int pf_depth_update(float* d_s, float* w_s, const float* d_m, const float* w_m, const unsigned char* disagree, const int* flags,
                               int* seg, int B, int H, int W, float tol_log2, float decay, float w_max, void* stream) {
    PfDepthUpdArgs a;
    const int rc = pf_depth_update_check(d_s, w_s, d_m, w_m, disagree, flags, seg, B, H, W, tol_log2, decay, w_max, a);
    if (rc != PF_OK) return rc;
    if (pf_depth_quads(a))
        hipLaunchKernelGGL(pf_du4_kernel, dim3(pf_rp_blocks((long)H * W / 4), (unsigned)B), dim3(kBlock), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(pf_du_kernel, dim3(pf_rp_blocks((long)H * W), (unsigned)B), dim3(kBlock), 0, (hipStream_t)stream, a);
    const int rl = (int)hipGetLastError();
    if (rl != 0) return rl;
    hipLaunchKernelGGL(pf_du_seg_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}
