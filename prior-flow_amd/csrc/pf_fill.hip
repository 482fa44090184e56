// Push-pull hole filling on the device: the statement and every per-thread phase are pf_fill.h.  Everything
// runs on the stream it is given, reads nothing on the host, allocates nothing, uses no atomics and no memset; scratch may hold
// anything on entry (every cell is written before it is read).
//
// The level-by-level form, one launch per step (2 L + 2 launches for an image with L pulls):
//   pf_fill_prepare_kernel   one thread per pixel: w0.
//   pf_fill_pull_kernel      one thread per coarse cell.
//   pf_fill_push_kernel      one thread per fine cell; the apex step when there is no coarse level.
// The fused form behind pf_fill_pushpull, three launches whenever the levels above the fifth fit the apex kernel's LDS (about
// 600 000 pixels at C = 4, 1.5 million at C = 1; pf_fill_plan):
//   pf_fill_pulltile_kernel  a workgroup of 256 owns a 32 x 64 tile of level 0: w0 on the fly, levels 1..5 of the tile (16 x 32 down
//     to 1 x 2 cells) reduced through LDS and written to scratch.  A wave reads 2 x 64 consecutive pixels of two rows per level-1
//     row of 32 cells.
//   pf_fill_apex_kernel      one workgroup of 1024 per image: streams level S (5: 16 x 32 cells at 512 x 1024) from scratch, pulls
//     to 1 x 1 in LDS, writes empty, pushes back down in LDS and fills level S in place.
//   pf_fill_pushtile_kernel  a workgroup of 256 produces a 32 x 64 tile of out: the regions of the levels 5 .. 1 around the tile
//     in LDS (two cells of margin, columns modulo the level's width), then the tile itself, a wave on 64 consecutive x of a row.
// Larger maps run pf_fill_pull_kernel / pf_fill_push_kernel for the levels between the tile kernels and the apex kernel.
// The arithmetic is written without branches around loads (pf_fill_pull_cell, pf_fill_push_cell): a thread's loads are in flight
// together, which is what the one workgroup of the apex kernel lives on.
//
// Every index is a cell inside its level: a tap is wrapped or clamped before it is used, a region position is cut to the region
// (PfFillRegionMap), a tile cell outside the map is skipped.
#include "pf_fill.h"

namespace {
constexpr int kBlock = 256;

__global__ void __launch_bounds__(kBlock) pf_fill_prepare_kernel(const PfFillPrepArgs a) {
    const long n = (long)blockIdx.x * kBlock + threadIdx.x;
    if (n < (long)a.H * a.W) pf_fill_prepare_pixel(a, (long)blockIdx.y, n);
}
__global__ void __launch_bounds__(kBlock) pf_fill_pull_kernel(const PfFillPullArgs a) {
    const long n = (long)blockIdx.x * kBlock + threadIdx.x;
    if (n < (long)a.hc * a.wc) pf_fill_pull_item(a, (long)blockIdx.y, n);
}
__global__ void __launch_bounds__(kBlock) pf_fill_push_kernel(const PfFillPushArgs a) {
    const long n = (long)blockIdx.x * kBlock + threadIdx.x;
    if (n < (long)a.hf * a.wf) pf_fill_push_item(a, (long)blockIdx.y, n);
}

__device__ __forceinline__ void pf_fill_tile_origin(const PfFillArgs& a, int& ty0, int& tx0) {
    const int tiles_x = (a.W + PF_FILL_TW - 1) / PF_FILL_TW;
    ty0 = ((int)blockIdx.x / tiles_x) * PF_FILL_TH;
    tx0 = ((int)blockIdx.x % tiles_x) * PF_FILL_TW;
}
__global__ void __launch_bounds__(PF_FILL_THREADS) pf_fill_pulltile_kernel(const PfFillArgs a) {
    __shared__ float lds[PF_FILL_PT_FLOATS];
    int ty0, tx0;
    pf_fill_tile_origin(a, ty0, tx0);
    for (int k = 1; k <= a.P; ++k) {
        pf_fill_pulltile_phase(a, lds, (long)blockIdx.y, ty0, tx0, k, (int)threadIdx.x);
        __syncthreads();
    }
}
__global__ void __launch_bounds__(PF_FILL_APEX_THREADS) pf_fill_apex_kernel(const PfFillArgs a) {
    __shared__ float lds[PF_FILL_APEX_FLOATS];
    __shared__ PfFillLevel tab[PF_FILL_MAX_LEVELS + 1];
    const long b = blockIdx.x;
    const int tid = threadIdx.x;
    if (tid >= a.S && tid <= a.L) tab[tid] = pf_fill_apex_level(a, lds, b, tid);
    __syncthreads();
    for (int l = a.S; l < a.L; ++l) {
        pf_fill_apex_pull(a, tab, l, tid);
        __syncthreads();
    }
    if (tid == 0) pf_fill_apex_top(a, tab, b);
    __syncthreads();
    for (int l = a.L - 1; l >= a.S; --l) {
        pf_fill_apex_push(a, tab, l, tid);
        __syncthreads();
    }
}
__global__ void __launch_bounds__(PF_FILL_THREADS) pf_fill_pushtile_kernel(const PfFillArgs a) {
    __shared__ float lds[PF_FILL_PU_FLOATS];
    int ty0, tx0;
    pf_fill_tile_origin(a, ty0, tx0);
    const long b = blockIdx.y;
    const int tid = threadIdx.x;
    pf_fill_pushtile_load(a, lds, b, ty0, tx0, tid);
    __syncthreads();
    for (int l = a.P - 1; l >= 1; --l) {
        pf_fill_pushtile_level(a, lds, b, ty0, tx0, l, tid);
        __syncthreads();
    }
    pf_fill_pushtile_out(a, lds, b, ty0, tx0, tid);
}

unsigned pf_fill_blocks(long items) { return (unsigned)((items + kBlock - 1) / kBlock); }

int pf_fill_launch_prepare(const PfFillPrepArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(pf_fill_prepare_kernel, dim3(pf_fill_blocks((long)a.H * a.W), (unsigned)a.B), dim3(kBlock), 0, st, a);
    return (int)hipGetLastError();
}
int pf_fill_launch_pull(const PfFillPullArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(pf_fill_pull_kernel, dim3(pf_fill_blocks((long)a.hc * a.wc), (unsigned)a.B), dim3(kBlock), 0, st, a);
    return (int)hipGetLastError();
}
int pf_fill_launch_push(const PfFillPushArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(pf_fill_push_kernel, dim3(pf_fill_blocks((long)a.hf * a.wf), (unsigned)a.B), dim3(kBlock), 0, st, a);
    return (int)hipGetLastError();
}
// level l of the scratch of a fused call: values and weights of all images
void pf_fill_level_ptrs(const PfFillArgs& a, int l, float*& v, float*& w, int& h, int& wd) {
    pf_fill_dims(a.H, a.W, l, h, wd);
    v = a.scratch + pf_fill_level_off(a.B, a.C, a.H, a.W, l);
    w = v + (long)a.B * a.C * h * wd;
}
}  // namespace

extern "C" int pf_fill_levels(int H, int W) { return pf_fill_levels_of(H, W); }
extern "C" long pf_fill_bytes(int B, int C, int H, int W) { return pf_fill_bytes_of(B, C, H, W); }

extern "C" int pf_fill_prepare(const float* src, const unsigned char* hole, const float* weight, float* w0, int B, int C, int H, int W,
                               void* stream) {
    PfFillPrepArgs a;
    const int rc = pf_fill_prepare_check(src, hole, weight, w0, B, C, H, W, a);
    return rc != PF_OK ? rc : pf_fill_launch_prepare(a, (hipStream_t)stream);
}
extern "C" int pf_fill_pull_level(const float* fine_v, const float* fine_w, float* coarse_v, float* coarse_w, int B, int C, int Hf, int Wf,
                                  void* stream) {
    PfFillPullArgs a;
    const int rc = pf_fill_pull_check(fine_v, fine_w, coarse_v, coarse_w, B, C, Hf, Wf, a);
    return rc != PF_OK ? rc : pf_fill_launch_pull(a, (hipStream_t)stream);
}
extern "C" int pf_fill_push_level(const float* coarse_u, const float* fine_v, const float* fine_w, float* out, unsigned char* empty, int B,
                                  int C, int Hf, int Wf, void* stream) {
    PfFillPushArgs a;
    const int rc = pf_fill_push_check(coarse_u, fine_v, fine_w, out, empty, B, C, Hf, Wf, a);
    return rc != PF_OK ? rc : pf_fill_launch_push(a, (hipStream_t)stream);
}

// the launches of the fused form; stages: bit 0 the pull tiles, bit 1 the apex (with the level-by-level launches around it on a
// large map), bit 2 the push tiles
static int pf_fill_run(const PfFillArgs& a, int stages, hipStream_t st) {
    const int B = a.B, C = a.C;
    int e;
    if (a.L == 0) {                                              // a 1 x 1 image is its own apex
        if (!(stages & 2)) return PF_OK;
        PfFillPrepArgs p;
        p.src = a.src; p.hole = a.hole; p.weight = a.weight; p.w0 = a.scratch; p.B = B; p.C = C; p.H = 1; p.W = 1;
        if ((e = pf_fill_launch_prepare(p, st)) != 0) return e;
        PfFillPushArgs q;
        q.coarse_u = nullptr; q.fine_v = a.src; q.fine_w = a.scratch; q.out = a.out; q.empty = a.empty;
        q.B = B; q.C = C; q.hf = q.wf = q.hc = q.wc = 1;
        return pf_fill_launch_push(q, st);
    }
    const long tiles = (long)((a.H + PF_FILL_TH - 1) / PF_FILL_TH) * ((a.W + PF_FILL_TW - 1) / PF_FILL_TW);     // < 2^30 / 2048 + H + W
    if (stages & 1) {
        hipLaunchKernelGGL(pf_fill_pulltile_kernel, dim3((unsigned)tiles, (unsigned)B), dim3(PF_FILL_THREADS), 0, st, a);
        if ((e = (int)hipGetLastError()) != 0) return e;
    }
    if (stages & 2) {
        for (int l = a.P; l < a.S; ++l) {
            PfFillPullArgs p;
            float *fv, *fw, *cv, *cw;
            pf_fill_level_ptrs(a, l, fv, fw, p.hf, p.wf);
            pf_fill_level_ptrs(a, l + 1, cv, cw, p.hc, p.wc);
            p.fine_v = fv; p.fine_w = fw; p.coarse_v = cv; p.coarse_w = cw; p.B = B; p.C = C;
            if ((e = pf_fill_launch_pull(p, st)) != 0) return e;
        }
        hipLaunchKernelGGL(pf_fill_apex_kernel, dim3((unsigned)B), dim3(PF_FILL_APEX_THREADS), 0, st, a);
        if ((e = (int)hipGetLastError()) != 0) return e;
        for (int l = a.S - 1; l >= a.P; --l) {
            PfFillPushArgs q;
            float *fv, *fw, *cv, *cw;
            pf_fill_level_ptrs(a, l, fv, fw, q.hf, q.wf);
            pf_fill_level_ptrs(a, l + 1, cv, cw, q.hc, q.wc);
            q.coarse_u = cv; q.fine_v = fv; q.fine_w = fw; q.out = fv; q.empty = nullptr; q.B = B; q.C = C;
            if ((e = pf_fill_launch_push(q, st)) != 0) return e;
        }
    }
    if (stages & 4) {
        hipLaunchKernelGGL(pf_fill_pushtile_kernel, dim3((unsigned)tiles, (unsigned)B), dim3(PF_FILL_THREADS), 0, st, a);
        return (int)hipGetLastError();
    }
    return PF_OK;
}

extern "C" int pf_fill_pushpull(const float* src, const unsigned char* hole, const float* weight, float* out, unsigned char* empty,
                                void* scratch, int B, int C, int H, int W, void* stream) {
    PfFillArgs a;
    const int rc = pf_fill_pushpull_check(src, hole, weight, out, empty, scratch, B, C, H, W, a);
    return rc != PF_OK ? rc : pf_fill_run(a, 7, (hipStream_t)stream);
}
extern "C" int pf_fill_stage(const float* src, const unsigned char* hole, const float* weight, float* out, unsigned char* empty,
                             void* scratch, int B, int C, int H, int W, int stage, void* stream) {
    PfFillArgs a;
    const int rc = pf_fill_pushpull_check(src, hole, weight, out, empty, scratch, B, C, H, W, a);
    if (rc != PF_OK) return rc;
    if (stage < 0 || stage > 2) return PF_ERR_BAD_ARG;
    return pf_fill_run(a, 1 << stage, (hipStream_t)stream);
}
