// Host emulation of pf_fill_* -- TEST INFRASTRUCTURE ONLY (its own library, libpf_emu_fill.so).  The arithmetic, the geometry, the
// per-thread phases of the fused kernels and the argument checks are prior-flow_amd/csrc/pf_fill.h, the file the device kernels
// compile; a launch is restated as a loop over its grid, a workgroup as a loop over its threads per phase (where the device has a
// barrier), its LDS as an array that holds NaN when the workgroup starts.  The product never loads this library.
//
// The library also holds pf_emu_splat.cpp's and pf_emu_reproject.cpp's entry points, so that one handle serves a FrameInterpolator,
// a Reprojector or an Odometry with its DepthPropagator and the HoleFiller behind them.  Both files bring a visiting order and a
// pf_version of their own: the splat file's are renamed here, the reprojection file's are the library's.
#include <limits>
#include <vector>

#include "pf_fill.h"
#define g_order pf_emu_splat_g_order
#define pf_version pf_emu_splat_version
#include "pf_emu_splat.cpp"
#undef g_order
#undef pf_version
#include "pf_emu_reproject.cpp"

extern "C" int pf_fill_levels(int H, int W) { return pf_fill_levels_of(H, W); }
extern "C" long pf_fill_bytes(int B, int C, int H, int W) { return pf_fill_bytes_of(B, C, H, W); }

static void run_prepare(const PfFillPrepArgs& a) {
    for (long b = 0; b < a.B; ++b)
        for (long n = 0; n < (long)a.H * a.W; ++n) pf_fill_prepare_pixel(a, b, n);
}
static void run_pull(const PfFillPullArgs& a) {
    for (long b = 0; b < a.B; ++b)
        for (long n = 0; n < (long)a.hc * a.wc; ++n) pf_fill_pull_item(a, b, n);
}
static void run_push(const PfFillPushArgs& a) {
    for (long b = 0; b < a.B; ++b)
        for (long n = 0; n < (long)a.hf * a.wf; ++n) pf_fill_push_item(a, b, n);
}

extern "C" int pf_fill_prepare(const float* src, const unsigned char* hole, const float* weight, float* w0, int B, int C, int H, int W,
                               void*) {
    PfFillPrepArgs a;
    const int rc = pf_fill_prepare_check(src, hole, weight, w0, B, C, H, W, a);
    if (rc != PF_OK) return rc;
    run_prepare(a);
    return PF_OK;
}
extern "C" int pf_fill_pull_level(const float* fine_v, const float* fine_w, float* coarse_v, float* coarse_w, int B, int C, int Hf, int Wf,
                                  void*) {
    PfFillPullArgs a;
    const int rc = pf_fill_pull_check(fine_v, fine_w, coarse_v, coarse_w, B, C, Hf, Wf, a);
    if (rc != PF_OK) return rc;
    run_pull(a);
    return PF_OK;
}
extern "C" int pf_fill_push_level(const float* coarse_u, const float* fine_v, const float* fine_w, float* out, unsigned char* empty, int B,
                                  int C, int Hf, int Wf, void*) {
    PfFillPushArgs a;
    const int rc = pf_fill_push_check(coarse_u, fine_v, fine_w, out, empty, B, C, Hf, Wf, a);
    if (rc != PF_OK) return rc;
    run_push(a);
    return PF_OK;
}

static void level_ptrs(const PfFillArgs& a, int l, float*& v, float*& w, int& h, int& wd) {
    pf_fill_dims(a.H, a.W, l, h, wd);
    v = a.scratch + pf_fill_level_off(a.B, a.C, a.H, a.W, l);
    w = v + (long)a.B * a.C * h * wd;
}

// the launches of the fused form; stages: bit 0 the pull tiles, bit 1 the apex (with the level-by-level launches around it), bit 2
// the push tiles
static void run_fused(const PfFillArgs& a, int stages) {
    const int B = a.B, C = a.C, H = a.H, W = a.W;
    const float nan = std::numeric_limits<float>::quiet_NaN();
    if (a.L == 0) {
        if (!(stages & 2)) return;
        PfFillPrepArgs p;
        p.src = a.src; p.hole = a.hole; p.weight = a.weight; p.w0 = a.scratch; p.B = B; p.C = C; p.H = 1; p.W = 1;
        run_prepare(p);
        PfFillPushArgs q;
        q.coarse_u = nullptr; q.fine_v = a.src; q.fine_w = a.scratch; q.out = a.out; q.empty = a.empty;
        q.B = B; q.C = C; q.hf = q.wf = q.hc = q.wc = 1;
        run_push(q);
        return;
    }
    const int tiles_x = (W + PF_FILL_TW - 1) / PF_FILL_TW, tiles_y = (H + PF_FILL_TH - 1) / PF_FILL_TH;
    std::vector<float> lds;
    for (long b = 0; b < B && (stages & 1); ++b)
        for (int t = 0; t < tiles_x * tiles_y; ++t) {
            const int ty0 = (t / tiles_x) * PF_FILL_TH, tx0 = (t % tiles_x) * PF_FILL_TW;
            lds.assign(PF_FILL_PT_FLOATS, nan);
            for (int k = 1; k <= a.P; ++k)
                for (int tid = 0; tid < PF_FILL_THREADS; ++tid) pf_fill_pulltile_phase(a, lds.data(), b, ty0, tx0, k, tid);
        }
    for (int l = a.P; l < a.S && (stages & 2); ++l) {
        PfFillPullArgs p;
        float *fv, *fw, *cv, *cw;
        level_ptrs(a, l, fv, fw, p.hf, p.wf);
        level_ptrs(a, l + 1, cv, cw, p.hc, p.wc);
        p.fine_v = fv; p.fine_w = fw; p.coarse_v = cv; p.coarse_w = cw; p.B = B; p.C = C;
        run_pull(p);
    }
    for (long b = 0; b < B && (stages & 2); ++b) {
        lds.assign(PF_FILL_APEX_FLOATS, nan);
        std::vector<PfFillLevel> tab(PF_FILL_MAX_LEVELS + 1);
        for (int tid = a.S; tid <= a.L; ++tid) tab[tid] = pf_fill_apex_level(a, lds.data(), b, tid);
        for (int l = a.S; l < a.L; ++l)
            for (int tid = 0; tid < PF_FILL_APEX_THREADS; ++tid) pf_fill_apex_pull(a, tab.data(), l, tid);
        pf_fill_apex_top(a, tab.data(), b);
        for (int l = a.L - 1; l >= a.S; --l)
            for (int tid = 0; tid < PF_FILL_APEX_THREADS; ++tid) pf_fill_apex_push(a, tab.data(), l, tid);
    }
    for (int l = a.S - 1; l >= a.P && (stages & 2); --l) {
        PfFillPushArgs q;
        float *fv, *fw, *cv, *cw;
        level_ptrs(a, l, fv, fw, q.hf, q.wf);
        level_ptrs(a, l + 1, cv, cw, q.hc, q.wc);
        q.coarse_u = cv; q.fine_v = fv; q.fine_w = fw; q.out = fv; q.empty = nullptr; q.B = B; q.C = C;
        run_push(q);
    }
    for (long b = 0; b < B && (stages & 4); ++b)
        for (int t = 0; t < tiles_x * tiles_y; ++t) {
            const int ty0 = (t / tiles_x) * PF_FILL_TH, tx0 = (t % tiles_x) * PF_FILL_TW;
            lds.assign(PF_FILL_PU_FLOATS, nan);
            for (int tid = 0; tid < PF_FILL_THREADS; ++tid) pf_fill_pushtile_load(a, lds.data(), b, ty0, tx0, tid);
            for (int l = a.P - 1; l >= 1; --l)
                for (int tid = 0; tid < PF_FILL_THREADS; ++tid) pf_fill_pushtile_level(a, lds.data(), b, ty0, tx0, l, tid);
            for (int tid = 0; tid < PF_FILL_THREADS; ++tid) pf_fill_pushtile_out(a, lds.data(), b, ty0, tx0, tid);
        }
}

extern "C" int pf_fill_pushpull(const float* src, const unsigned char* hole, const float* weight, float* out, unsigned char* empty,
                                void* scratch, int B, int C, int H, int W, void*) {
    PfFillArgs a;
    const int rc = pf_fill_pushpull_check(src, hole, weight, out, empty, scratch, B, C, H, W, a);
    if (rc != PF_OK) return rc;
    run_fused(a, 7);
    return PF_OK;
}
extern "C" int pf_fill_stage(const float* src, const unsigned char* hole, const float* weight, float* out, unsigned char* empty,
                             void* scratch, int B, int C, int H, int W, int stage, void*) {
    PfFillArgs a;
    const int rc = pf_fill_pushpull_check(src, hole, weight, out, empty, scratch, B, C, H, W, a);
    if (rc != PF_OK) return rc;
    if (stage < 0 || stage > 2) return PF_ERR_BAD_ARG;
    run_fused(a, 1 << stage);
    return PF_OK;
}

// the split of the levels of a shape, for the tests: out = {L, P, S}
extern "C" void pf_emu_fill_plan(int C, int H, int W, int* out) { pf_fill_plan(C, H, W, out[0], out[1], out[2]); }
