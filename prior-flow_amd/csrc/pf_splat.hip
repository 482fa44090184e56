// Forward softmax splatting on the device: two launches per call, the per-pixel arithmetic is pf_splat.h.
//
//   pf_splat_acc_kernel     one thread per SOURCE pixel, two pixels per thread      grid (tiles of 8 x 64 pixels, njobs, B)
//     a wave holds 64 consecutive pixels of a row; the job lies along blockIdx.y (its fields are scalar) and is picked with
//     constant indices.  The adds are 64-bit integer atomics whose result is not read.  A workgroup's taps first meet in an
//     LDS window of kWinY x kWinX target cells per plane, placed where the tile's centre pixel lands (columns modulo the map
//     width: the panorama wraps); the cells that were touched then go to the sums [B][C+2][H][W] int64 as ONE global atomic
//     each, a row of the window as one contiguous run.  A tap outside the window (a flow that tears inside the tile) goes to
//     memory directly.  Integer adds commute, so where an add is made does not change a bit of the result.
//   pf_splat_res_kernel     one thread per TARGET pixel, or per four of them         grid (pixels / 256 or pixels / 1024, B)
//     reads the C + 2 sums, writes C floats and the hole byte and zeros over the sums: the sums are all-zero after a call.
//
// Every index is wrapped or range-checked before it is used (pf_splat_pixel_to converts a position to an integer only after the
// test that it is finite and nearer than 2^30; a window cell is addressed only after the unsigned range test, and a non-zero cell
// can only have come from a target inside the map), so neither kernel can touch memory outside its maps whatever the flow holds.
#include "pf_splat.h"

namespace {
constexpr int kBlock = 256;
constexpr int kTileY = 8, kTileX = 64;                  // source pixels of a workgroup: a wave takes rows w and w + 4
constexpr int kMarginY = 4, kMarginX = 8;
constexpr int kWinY = kTileY + 2 * kMarginY, kWinX = kTileX + 2 * kMarginX, kCells = kWinY * kWinX;      // 16 x 80
constexpr int kPlanes = 6;                              // C + 2 <= 6: 61 440 bytes of LDS
constexpr float kNear = 268435456.f;                   // 2^28: a window is placed only this near to the map

// the window in front of the direct sink: ox in [0, W), so xx - ox lies in (-W, W).  The window pointer carries its address space:
// with a generic pointer hipcc merges the two branches below into ONE flat atomic on a selected address
typedef __attribute__((address_space(3))) unsigned long long PfSplatLds;
struct PfSplatWindow {
    PfSplatLds* win; int ox, oy, W; PfSplatDirect direct;
    __device__ __forceinline__ void add(int plane, int yy, int xx, long long v) const {
        int xr = xx - ox;
        xr = xr < 0 ? xr + W : xr;
        const int yr = yy - oy;
        if ((unsigned)xr < (unsigned)kWinX && (unsigned)yr < (unsigned)kWinY)
            __hip_atomic_fetch_add(win + (plane * kCells + yr * kWinX + xr), (unsigned long long)v, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_WORKGROUP);
        else
            direct.add(plane, yy, xx, v);
    }
};

__global__ void __launch_bounds__(kBlock) pf_splat_acc_kernel(const PfSplatAccArgs a) {
    __shared__ unsigned long long win[kPlanes * kCells];
    const int tid = threadIdx.x, planes = a.C + 2;
    for (int i = tid; i < planes * kCells; i += kBlock) win[i] = 0;
    const int tiles_x = (a.W + kTileX - 1) / kTileX;
    const int ty0 = ((int)blockIdx.x / tiles_x) * kTileY, tx0 = ((int)blockIdx.x % tiles_x) * kTileX;
    const PfSplatJob q = pf_splat_pick(a, (int)blockIdx.y);
    const long b = blockIdx.z, N = (long)a.H * a.W;
    // the window's origin: where the tile's centre pixel lands (the tile's own place when that is not finite), less the margins
    const int cy = min(ty0 + kTileY / 2, a.H - 1), cx = min(tx0 + kTileX / 2, a.W - 1);
    const float* fl = q.flow + b * 2 * N + ((long)cy * a.W + cx);
    const float qx = (float)cx + q.tau * fl[0], qy = (float)cy + q.tau * fl[N];
    const bool ok = fabsf(qx) < kNear && fabsf(qy) < kNear;           // a NaN compares false; yy - oy stays inside an int
    const int ix = ok ? (int)floorf(qx) : cx, iy = ok ? (int)floorf(qy) : cy;
    PfSplatWindow sink;
    sink.win = (PfSplatLds*)win; sink.W = a.W; sink.direct = pf_splat_direct(a, b);
    sink.oy = iy - (cy - ty0) - kMarginY;
    int ox = (ix - (cx - tx0) - kMarginX) % a.W;
    sink.ox = ox < 0 ? ox + a.W : ox;
    __syncthreads();
    const int x = tx0 + (tid & 63);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int y = ty0 + (tid >> 6) + 4 * r;
        if (y < a.H && x < a.W) pf_splat_pixel_to(q, a, b, y, x, sink);
    }
    __syncthreads();
    for (int i = tid; i < planes * kCells; i += kBlock) {
        const unsigned long long v = win[i];
        if (v == 0) continue;
        const int plane = i / kCells, cell = i - plane * kCells;
        const int yr = cell / kWinX, xr = cell - yr * kWinX;
        // a filled cell came from a target (yy, xx) inside the map with xr = (xx - ox) mod W < W: this is that target again
        sink.direct.add(plane, sink.oy + yr, (sink.ox + xr) % a.W, (long long)v);
    }
}
__global__ void __launch_bounds__(kBlock) pf_splat_res_kernel(const PfSplatResArgs a) {
    const int pix = blockIdx.x * kBlock + threadIdx.x;
    if (pix < a.H * a.W) pf_splat_resolve_pixel(a, (long)blockIdx.y, pix);
}
__global__ void __launch_bounds__(kBlock) pf_splat_res4_kernel(const PfSplatResArgs a) {
    const int quad = blockIdx.x * kBlock + threadIdx.x;
    if (quad < a.H * a.W / 4) pf_splat_resolve_quad(a, (long)blockIdx.y, 4L * quad);
}
unsigned pf_splat_blocks(long items) { return (unsigned)((items + kBlock - 1) / kBlock); }
}  // namespace

extern "C" long pf_splat_scratch_bytes(int B, int C, int H, int W) { return pf_splat_bytes(B, C, H, W); }

extern "C" int pf_splat_accumulate(const pf_splat_job* jobs, int njobs, void* acc, int B, int C, int H, int W, float alpha,
                                   float zmax, float vmax, void* stream) {
    PfSplatAccArgs a;
    const int rc = pf_splat_accumulate_check(jobs, njobs, acc, B, C, H, W, alpha, zmax, vmax, a);
    if (rc != PF_OK) return rc;
    const long tiles = (long)((H + kTileY - 1) / kTileY) * ((W + kTileX - 1) / kTileX);         // < 2^30 / 64 + H + W
    hipLaunchKernelGGL(pf_splat_acc_kernel, dim3((unsigned)tiles, (unsigned)njobs, (unsigned)B), dim3(kBlock), 0,
                       (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

extern "C" int pf_splat_resolve(void* acc, float* out, unsigned char* hole, const float* fill0, const float* fill1, float fill_t,
                                float cmin, int njobs, int B, int C, int H, int W, float vmax, void* stream) {
    PfSplatResArgs a;
    const int rc = pf_splat_resolve_check(acc, out, hole, fill0, fill1, fill_t, cmin, njobs, B, C, H, W, vmax, a);
    if (rc != PF_OK) return rc;
    if (pf_splat_quads(a))
        hipLaunchKernelGGL(pf_splat_res4_kernel, dim3(pf_splat_blocks((long)H * W / 4), (unsigned)B), dim3(kBlock), 0,
                           (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(pf_splat_res_kernel, dim3(pf_splat_blocks((long)H * W), (unsigned)B), dim3(kBlock), 0,
                           (hipStream_t)stream, a);
    return (int)hipGetLastError();
}
