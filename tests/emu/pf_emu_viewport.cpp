// Host emulation of pf_viewport_image / pf_viewport_flow / pf_cubemap_to_erp -- TEST INFRASTRUCTURE ONLY (its own library,
// libpf_emu_viewport.so).  The per-pixel arithmetic and the argument checks are prior-flow_amd/csrc/pf_viewport.h, the file the
// device kernels compile; a launch is restated as a loop over its grid.  The product never loads this library.
#include "pf_viewport.h"

extern "C" int pf_viewport_image(const void* in, void* out, const float* views_host, int V, int B, int C, int H, int W, int form,
                                 void*) {
    PfViewImageArgs a;
    const int rc = pf_viewport_image_check(in, out, views_host, V, B, C, H, W, form, a);
    if (rc != PF_OK) return rc;
    for (int bv = 0; bv < B * V; ++bv)
        for (int pix = 0; pix < a.h * a.w; ++pix) pf_vp_image_pixel(a, bv, pix);
    return PF_OK;
}

extern "C" int pf_viewport_flow(const float* flow, const float* views_host, int V, float* out, unsigned char* valid, int B, int H,
                                int W, float min_forward, void*) {
    PfViewFlowArgs a;
    const int rc = pf_viewport_flow_check(flow, views_host, V, out, valid, B, H, W, min_forward, a);
    if (rc != PF_OK) return rc;
    for (int bv = 0; bv < B * V; ++bv)
        for (int pix = 0; pix < a.h * a.w; ++pix) pf_vp_flow_pixel(a, bv, pix);
    return PF_OK;
}

extern "C" int pf_cubemap_to_erp(const float* faces, float* out, int B, int C, int s, int H, int W, void*) {
    PfCubeErpArgs a;
    const int rc = pf_cubemap_to_erp_check(faces, out, B, C, s, H, W, a);
    if (rc != PF_OK) return rc;
    for (int b = 0; b < B; ++b)
        for (int pix = 0; pix < H * W; ++pix) pf_vp_cube_pixel(a, b, pix);
    return PF_OK;
}

// the face of a direction (pf_vp_cube_face), callable on its own: an exact tie never falls on a pixel centre
extern "C" int pf_emu_cube_face(float x, float y, float z) { PfVec3 d; d.x = x; d.y = y; d.z = z; return pf_vp_cube_face(d); }
extern "C" const char* pf_version(void) { return "priorflow viewport host emulation (tests only)"; }
