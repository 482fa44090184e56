// Perspective viewports and cube maps of ERP frames and ERP flow on the device: three launches, one thread
// per output pixel, the ray / ERP position / taps of a pixel computed once for all its channels.
//
//   pf_vp_image_kernel   ERP -> V views, fp32 planes or channel-last bytes           grid (pixels / 256, B * V)
//   pf_vp_flow_kernel    ERP flow -> pinhole flow + valid of V views                 grid (pixels / 256, B * V)
//   pf_vp_cube_kernel    six cube faces -> ERP                                       grid (pixels / 256, B)
//
// The view table (at most PF_VIEW_MAX rows of R, f, h, w) is a kernel argument: nothing is copied to the device and a call can be
// captured.  The per-pixel arithmetic is pf_viewport.h.
#include "pf_viewport.h"

namespace {
constexpr int kBlock = 256;

__global__ void __launch_bounds__(kBlock) pf_vp_image_kernel(const PfViewImageArgs a) {
    const int pix = blockIdx.x * kBlock + threadIdx.x;
    if (pix < a.h * a.w) pf_vp_image_pixel(a, (int)blockIdx.y, pix);
}
__global__ void __launch_bounds__(kBlock) pf_vp_flow_kernel(const PfViewFlowArgs a) {
    const int pix = blockIdx.x * kBlock + threadIdx.x;
    if (pix < a.h * a.w) pf_vp_flow_pixel(a, (int)blockIdx.y, pix);
}
__global__ void __launch_bounds__(kBlock) pf_vp_cube_kernel(const PfCubeErpArgs a) {
    const int pix = blockIdx.x * kBlock + threadIdx.x;
    if (pix < a.H * a.W) pf_vp_cube_pixel(a, (int)blockIdx.y, pix);
}
unsigned pf_vp_blocks(long pixels) { return (unsigned)((pixels + kBlock - 1) / kBlock); }
}  // namespace

extern "C" int pf_viewport_image(const void* in, void* out, const float* views_host, int V, int B, int C, int H, int W, int form,
                                 void* stream) {
    PfViewImageArgs a;
    const int rc = pf_viewport_image_check(in, out, views_host, V, B, C, H, W, form, a);
    if (rc != PF_OK) return rc;
    hipLaunchKernelGGL(pf_vp_image_kernel, dim3(pf_vp_blocks((long)a.h * a.w), (unsigned)(B * V)), dim3(kBlock), 0,
                       (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

extern "C" int pf_viewport_flow(const float* flow, const float* views_host, int V, float* out, unsigned char* valid, int B, int H,
                                int W, float min_forward, void* stream) {
    PfViewFlowArgs a;
    const int rc = pf_viewport_flow_check(flow, views_host, V, out, valid, B, H, W, min_forward, a);
    if (rc != PF_OK) return rc;
    hipLaunchKernelGGL(pf_vp_flow_kernel, dim3(pf_vp_blocks((long)a.h * a.w), (unsigned)(B * V)), dim3(kBlock), 0,
                       (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

extern "C" int pf_cubemap_to_erp(const float* faces, float* out, int B, int C, int s, int H, int W, void* stream) {
    PfCubeErpArgs a;
    const int rc = pf_cubemap_to_erp_check(faces, out, B, C, s, H, W, a);
    if (rc != PF_OK) return rc;
    hipLaunchKernelGGL(pf_vp_cube_kernel, dim3(pf_vp_blocks((long)H * W), (unsigned)B), dim3(kBlock), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}
