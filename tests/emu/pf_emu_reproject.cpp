// Host emulation of pf_reproj_project / pf_zsplat_front / pf_zsplat_accumulate / pf_zsplat_resolve / pf_depth_update -- TEST
// INFRASTRUCTURE ONLY (its own library, libpf_emu_reproject.so).  The per-pixel arithmetic, the scales and the argument checks are
// prior-flow_amd/csrc/pf_reproject.h, the file the device kernels compile; a launch is restated as a loop over its grid, an
// atomic add or maximum as a plain one.  The product never loads this library.
//
// pf_emu_odo_order (pf_emu_odometry.cpp) also picks the order in which the front and the accumulate loops visit the source pixels
// of an image: 0 row by row, 1 reversed, any other value a fixed pseudo-random permutation seeded with it.  Maxima and integer
// adds commute, so front and the sums must not notice (tests/test_reproject_host.py).  The library holds pf_emu_odometry.cpp's
// entry points as well, so that one handle serves an Odometry and the DepthPropagator behind it.
#include "pf_reproject.h"
// the trajectory and pose entry points, the visiting order (g_order, visit_order) and pf_version
#include "pf_emu_odometry.cpp"

extern "C" int pf_reproj_project(const float* inv_depth, const float* weight, const unsigned char* mask, const float* R, const float* T,
                                 float* flow, float* d_new, unsigned char* valid, int B, int H, int W, float n_min, void*) {
    PfReprojArgs a;
    const int rc = pf_reproj_project_check(inv_depth, weight, mask, R, T, flow, d_new, valid, B, H, W, n_min, a);
    if (rc != PF_OK) return rc;
    for (long b = 0; b < B; ++b) {
        PfVec3 Tb;
        Tb.x = T[b * 3]; Tb.y = T[b * 3 + 1]; Tb.z = T[b * 3 + 2];
        for (int y = 0; y < H; ++y) {
            float cp, sp;
            pf_ego_row(y, H, cp, sp);
            for (int x = 0; x < W; ++x) pf_reproj_pixel(a, R + b * 9, Tb, b, y, x, cp, sp);
        }
    }
    return PF_OK;
}

extern "C" long pf_zsplat_bytes(int B, int C, int H, int W) { return pf_zsplat_acc_bytes(B, C, H, W); }

extern "C" int pf_zsplat_front(const float* src, const float* flow, const float* d, const float* weight, const unsigned char* valid,
                               void* front, int B, int C, int H, int W, float b_min, void*) {
    PfZsplatArgs a;
    const int rc = pf_zsplat_check(src, flow, d, weight, valid, front, nullptr, false, B, C, H, W, b_min, 0.f, 1.f, 1.f, 1.f, a);
    if (rc != PF_OK) return rc;
    const std::vector<long> order = visit_order((long)H * W);
    for (long b = 0; b < B; ++b)
        for (long n : order) pf_zsplat_front_pixel(a, b, (int)(n / W), (int)(n % W));
    return PF_OK;
}

extern "C" int pf_zsplat_accumulate(const float* src, const float* flow, const float* d, const float* weight, const unsigned char* valid,
                                    const void* front, void* acc, int B, int C, int H, int W, float b_min, float tol_log2, float w_max,
                                    float dmax, float vmax, void*) {
    PfZsplatArgs a;
    const int rc = pf_zsplat_check(src, flow, d, weight, valid, const_cast<void*>(front), acc, true, B, C, H, W, b_min, tol_log2, w_max,
                                   dmax, vmax, a);
    if (rc != PF_OK) return rc;
    const std::vector<long> order = visit_order((long)H * W);
    for (long b = 0; b < B; ++b)
        for (long n : order) pf_zsplat_acc_pixel(a, b, (int)(n / W), (int)(n % W));
    return PF_OK;
}

extern "C" int pf_zsplat_resolve(void* acc, void* front, float* out, float* d_out, float* w_out, unsigned char* hole, int B, int C, int H,
                                 int W, float cmin, float w_max, float dmax, float vmax, void*) {
    PfZsplatResArgs a;
    const int rc = pf_zsplat_resolve_check(acc, front, out, d_out, w_out, hole, B, C, H, W, cmin, w_max, dmax, vmax, a);
    if (rc != PF_OK) return rc;
    const long N = (long)H * W;
    const bool quads = pf_zsplat_quads(a);
    for (long b = 0; b < B; ++b) {
        if (quads) for (long n = 0; n < N; n += 4) pf_zsplat_resolve_quad(a, b, n);
        else for (long n = 0; n < N; ++n) pf_zsplat_resolve_pixel(a, b, n);
    }
    return PF_OK;
}

extern "C" int pf_depth_update(float* d_s, float* w_s, const float* d_m, const float* w_m, const unsigned char* disagree, const int* flags,
                               int* seg, int B, int H, int W, float tol_log2, float decay, float w_max, void*) {
    PfDepthUpdArgs a;
    const int rc = pf_depth_update_check(d_s, w_s, d_m, w_m, disagree, flags, seg, B, H, W, tol_log2, decay, w_max, a);
    if (rc != PF_OK) return rc;
    const long N = (long)H * W;
    const bool quads = pf_depth_quads(a);
    for (long b = 0; b < B; ++b) {
        if (quads) for (long n = 0; n < N; n += 4) pf_depth_update_quad(a, b, n);
        else for (long n = 0; n < N; ++n) pf_depth_update_pixel(a, b, n);
    }
    for (long b = 0; b < B; ++b) pf_depth_seg_image(a, b);
    return PF_OK;
}

// which form a resolve / an update of these maps takes (1: the quad form), for the tests of the element form
extern "C" int pf_emu_zsplat_quads(const void* acc, const void* front, const float* out, const float* d_out, const float* w_out,
                                   const unsigned char* hole, int W) {
    PfZsplatResArgs a;
    a.acc = (long long*)acc; a.front = (unsigned*)front; a.out = (float*)out; a.d_out = (float*)d_out; a.w_out = (float*)w_out;
    a.hole = (unsigned char*)hole; a.W = W;
    return pf_zsplat_quads(a) ? 1 : 0;
}
