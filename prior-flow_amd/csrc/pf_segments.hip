// Moving objects on the device: the statement is pf_segments.h.  Everything runs on the stream it is given,
// reads nothing on the host and allocates nothing.  An update is eight launches (pf_seg_label: 3, pf_seg_objects: 5), no memset.
//
//   pf_seg_label_local     one workgroup (256 threads) per 32 x 64 tile                    grid (tiles, B), 8448 bytes of LDS
//     a wave holds 64 consecutive pixels of one row: __ballot(set) is the row segment's bitmask, a pixel's run start follows from
//     bit operations, so a horizontal link costs no memory operation.  Vertical and diagonal links are LDS unions (atomic min),
//     and only the links that the runs of the two rows do not already imply are made.  Writes parent (global indices, -1 for
//     background) and zeroes the tile's cells of the area plane.
//   pf_seg_label_merge     one thread per tile-border pixel (column 0 is the seam), one workgroup per pole row
//     every read of parent is a relaxed agent-scope atomic load, every write an agent-scope atomic min: workgroups on different
//     XCDs share the array and there is no plain store to it in this kernel.
//   pf_seg_label_flatten   one thread per pixel, 1024 per workgroup: labels = root + 1, area[root] += cos phi (64-bit integer
//     atomic), combined first: the lanes of a wave that share its first root add up, the 16 waves combine those sums through LDS,
//     and every other root of a wave goes out as one atomic per distinct root.
//   pf_seg_rank_count / pf_seg_rank_scan / pf_seg_rank_assign   surviving roots per row (a wave per row, ballot), an exclusive scan
//     of the H counts by one workgroup per image (which also clears roots and sums), the dense numbers per row.
//   pf_seg_objects_accumulate   a grid sized by the CU count (1024 threads, two workgroups per CU); ids, keep; the sums go to LDS partial sums (M <= 512: 40 KiB) and
//     from there with one global 64-bit atomic per non-zero cell, or straight to global atomics for a larger M.
//   pf_seg_objects_resolve      one lane per object, fp64.
//
// Every index is a pixel index below H * W, a row below H, a column below W, an image below B or an object below M; labels and
// ranks are read only where these kernels wrote them in the same call, and a rank is compared with M before it indexes anything.
#include "pf_segments.h"

namespace {
constexpr int kBlock = 256, kWaves = kBlock / 64;
constexpr int kFlat = 1024;                                              // threads of the flatten and accumulate workgroups
constexpr int kLdsObjects = 512;                                        // M up to which the partial sums live in LDS

#define PF_SG_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT
#define PF_SG_RLX_WG __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP

struct SegLds {                                                          // a tile's cells in LDS, shared by the workgroup's waves
    int* p;
    __device__ int load(int i) const { return __hip_atomic_load(p + i, PF_SG_RLX_WG); }
    __device__ int min(int i, int v) const { return __hip_atomic_fetch_min(p + i, v, PF_SG_RLX_WG); }
};
struct SegGlobal {                                                       // parent in global memory, shared by every workgroup
    int* p;
    __device__ int load(int i) const { return __hip_atomic_load(p + i, PF_SG_RLX_AGENT); }
    __device__ int min(int i, int v) const { return __hip_atomic_fetch_min(p + i, v, PF_SG_RLX_AGENT); }
};
struct SegRead {                                                         // parent after the merge: nobody writes it any more
    const int* p;
    __device__ int load(int i) const { return p[i]; }
};

__global__ void __launch_bounds__(kBlock) pf_seg_tables_kernel(float* rows, float* cols, int H, int W) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    float c, s;
    if (i < H) { pf_seg_row(i, H, c, s); rows[2 * i] = c; rows[2 * i + 1] = s; }
    else if (i - H < W) { pf_seg_col(i - H, W, c, s); cols[2 * (i - H)] = c; cols[2 * (i - H) + 1] = s; }
}

__global__ void __launch_bounds__(kBlock) pf_seg_label_local(const PfSegLabelArgs a) {
    __shared__ int lab[PF_SG_TH * PF_SG_TW];
    __shared__ unsigned long long bits[PF_SG_TH];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int H = a.H, W = a.W, tiles_x = (W + PF_SG_TW - 1) / PF_SG_TW;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int x0 = tx * PF_SG_TW, y0 = ty * PF_SG_TH, x = x0 + lane;
    const long base = (long)blockIdx.y * H * W;
    for (int r = wave; r < PF_SG_TH; r += kWaves) {
        const int y = y0 + r;
        const bool set = x < W && y < H && pf_seg_set(a.mask[base + (long)y * W + x]);
        const unsigned long long bal = __ballot(set);
        const unsigned long long gaps = ~bal & ((1ull << lane) - 1ull);          // the clear bits below this lane
        const int start = gaps ? 64 - __clzll((long long)gaps) : 0;             // the run starts behind the highest of them
        lab[r * PF_SG_TW + lane] = set ? r * PF_SG_TW + start : -1;
        if (lane == 0) bits[r] = bal;
    }
    __syncthreads();
    const SegLds m{lab};
    for (int r = wave; r < PF_SG_TH; r += kWaves) {
        if (r == 0) continue;
        const unsigned long long cur = bits[r], up = bits[r - 1];
        if (!((cur >> lane) & 1ull)) continue;
        const int i = r * PF_SG_TW + lane, u = (r - 1) * PF_SG_TW + lane;
        const bool upc = (up >> lane) & 1ull, upl = lane > 0 && ((up >> (lane - 1)) & 1ull), upr = lane < 63 && ((up >> (lane + 1)) & 1ull);
        const bool left = lane > 0 && ((cur >> (lane - 1)) & 1ull), right = lane < 63 && ((cur >> (lane + 1)) & 1ull);
        // the pixel above: the left neighbour makes the same link when it and the pixel above it are set (one run above, one below)
        if (upc && !(left && upl)) pf_seg_unite(m, i, u);
        if (a.conn == 8 && !upc) {                               // with the pixel above set, both diagonals lie in its run
            if (upl && !left) pf_seg_unite(m, i, u - 1);         // a set left neighbour has (u - 1) straight above it
            if (upr && !right) pf_seg_unite(m, i, u + 1);        // a set right neighbour has (u + 1) straight above it
        }
    }
    __syncthreads();
    for (int r = wave; r < PF_SG_TH; r += kWaves) {
        const int y = y0 + r;
        if (x >= W || y >= H) continue;
        const int v = lab[r * PF_SG_TW + lane];
        int g = -1;
        if (v >= 0) {
            const int root = pf_seg_find(m, v);
            g = (y0 + root / PF_SG_TW) * W + x0 + root % PF_SG_TW;               // row-major in the tile as in the image: g <= own index
        }
        a.parent[base + (long)y * W + x] = g;
        a.area[base + (long)y * W + x] = 0;
    }
}

__global__ void __launch_bounds__(kBlock) pf_seg_label_merge(const PfSegLabelArgs a, long items, unsigned item_blocks) {
    __shared__ int anchor;
    const int H = a.H, W = a.W;
    const SegGlobal m{a.parent + (long)blockIdx.y * H * W};
    if (blockIdx.x < item_blocks) {
        const long t = (long)blockIdx.x * kBlock + threadIdx.x;
        if (t < items) pf_seg_merge_item(m, t, H, W, a.conn);
        return;
    }
    // a pole row: every set pixel with the row's first one
    const int off = (blockIdx.x - item_blocks == 0 ? 0 : H - 1) * W;
    if (threadIdx.x == 0) anchor = W;
    __syncthreads();
    for (int x = threadIdx.x; x < W; x += kBlock)
        if (m.load(off + x) >= 0) { atomicMin(&anchor, x); break; }
    __syncthreads();
    const int an = anchor;
    if (an >= W) return;
    for (int x = threadIdx.x; x < W; x += kBlock)
        if (x != an && m.load(off + x) >= 0) pf_seg_unite(m, off + x, off + an);
}

// `todo`: the lanes with a pending (root, q); one atomic per distinct root among them
__device__ void pf_seg_flush_roots(long long* area, int root, long long q, int lane) {
    unsigned long long todo = __ballot(root >= 0);
    while (todo) {
        const int first = __ffsll((long long)todo) - 1;
        const int r0 = __shfl(root, first);
        const bool mine = root == r0;
        long long s = mine ? q : 0;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d);
        if (lane == first) __hip_atomic_fetch_add(area + r0, s, PF_SG_RLX_AGENT);
        todo &= ~__ballot(mine);
    }
}
__global__ void __launch_bounds__(kFlat) pf_seg_label_flatten(const PfSegLabelArgs a) {
    __shared__ int wroot[kFlat / 64];
    __shared__ long long wsum[kFlat / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long N = (long)a.H * a.W, base = (long)blockIdx.y * N, n = (long)blockIdx.x * kFlat + threadIdx.x;
    int root = -1;
    long long q = 0;
    if (n < N) {
        const SegRead m{a.parent + base};
        if (m.load((int)n) >= 0) {
            root = pf_seg_find(m, (int)n);
            q = pf_seg_area_q(a.rows[2 * (int)(n / a.W)]);
        }
        a.labels[base + n] = root + 1;
    }
    // Atomics on one address run at about 13 ns each (measured: 56 us for the 4096 waves of the serpentine, 102 us for the 8200
    // wave-roots of the Bernoulli mask's giant cluster), so a large component must reach its cell in few of them.  The lanes that
    // share the wave's first root add up (every lane of the wave is here) and hand the sum to the workgroup through LDS, where
    // wave 0 combines the 16 of them; the wave's other roots go out one atomic per distinct root.
    const unsigned long long act = __ballot(root >= 0);
    const int r0 = act ? __shfl(root, __ffsll((long long)act) - 1) : -1;
    const bool mine = root >= 0 && root == r0;
    long long s = mine ? q : 0;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d);
    if (lane == 0) { wroot[wave] = r0; wsum[wave] = s; }
    pf_seg_flush_roots(a.area + base, mine ? -1 : root, q, lane);
    __syncthreads();
    if (wave == 0) {
        const bool have = lane < kFlat / 64;
        pf_seg_flush_roots(a.area + base, have ? wroot[lane] : -1, have ? wsum[lane] : 0, lane);
    }
}

// a wave per row: the surviving roots of the row
__global__ void __launch_bounds__(kBlock) pf_seg_rank_count(const PfSegObjArgs a) {
    const int lane = threadIdx.x & 63, y = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (y >= a.H) return;
    const long o = (long)blockIdx.y * a.H * a.W + (long)y * a.W;
    int cnt = 0;
    for (int x0 = 0; x0 < a.W; x0 += 64) {
        const int x = x0 + lane;
        cnt += __popcll(__ballot(x < a.W && pf_seg_survivor(a, o + x, y * a.W + x)));
    }
    if (lane == 0) a.rowcount[blockIdx.y * a.H + y] = cnt;
}
// one workgroup per image: rowbase = the exclusive scan of rowcount, count = the total; roots and sums cleared
__global__ void __launch_bounds__(kBlock) pf_seg_rank_scan(const PfSegObjArgs a) {
    __shared__ int part[kBlock];
    const int t = threadIdx.x, H = a.H;
    const long b = blockIdx.x;
    const int per = (H + kBlock - 1) / kBlock;
    const long lo_l = (long)t * per;
    const int lo = lo_l < H ? (int)lo_l : H, hi = lo_l + per < H ? (int)(lo_l + per) : H;
    int s = 0;
    for (int y = lo; y < hi; ++y) s += a.rowcount[b * H + y];
    part[t] = s;
    __syncthreads();
    for (int d = 1; d < kBlock; d <<= 1) {
        const int v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int run = part[t] - s;
    for (int y = lo; y < hi; ++y) { const int c = a.rowcount[b * H + y]; a.rowbase[b * H + y] = run; run += c; }
    if (t == 0) a.count[b] = part[kBlock - 1];
    for (int k = t; k < a.M; k += kBlock) a.roots[b * a.M + k] = -1;
    for (int k = t; k < a.M * PF_SEG_SUMS; k += kBlock) a.sums[b * a.M * PF_SEG_SUMS + k] = 0;
}
// a wave per row: rank of a surviving root = its number among the survivors, 0 everywhere else
__global__ void __launch_bounds__(kBlock) pf_seg_rank_assign(const PfSegObjArgs a) {
    const int lane = threadIdx.x & 63, y = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (y >= a.H) return;
    const long b = blockIdx.y, o = b * a.H * a.W + (long)y * a.W;
    int run = a.rowbase[b * a.H + y];
    for (int x0 = 0; x0 < a.W; x0 += 64) {
        const int x = x0 + lane;
        const bool in = x < a.W, sv = in && pf_seg_survivor(a, o + x, y * a.W + x);
        const unsigned long long bal = __ballot(sv);
        const int r = sv ? run + __popcll(bal & ((1ull << lane) - 1ull)) + 1 : 0;
        if (in) a.rank[o + x] = r;
        if (sv && r <= a.M) a.roots[b * a.M + (r - 1)] = y * a.W + x;
        run += __popcll(bal);
    }
}

template <bool kLds>
__global__ void __launch_bounds__(kFlat) pf_seg_objects_accumulate(const PfSegObjArgs a) {
    extern __shared__ long long part[];
    const long N = (long)a.H * a.W, b = blockIdx.y;
    const int cells = a.M * PF_SEG_SUMS, used = a.C > 0 ? 6 + a.C : 5;
    long long* g = a.sums + b * cells;
    if (kLds) {
        for (int k = threadIdx.x; k < cells; k += kFlat) part[k] = 0;
        __syncthreads();
    }
    for (long n = (long)blockIdx.x * kFlat + threadIdx.x; n < N; n += (long)gridDim.x * kFlat) {
        int id;
        pf_seg_pixel_ids(a, b, n, id);
        if (id <= 0) continue;
        const int y = (int)(n / a.W), x = (int)(n - (long)y * a.W);
        long long s[PF_SEG_SUMS];
        pf_seg_pixel_sums(a, b, y, x, s);
        long long* dst = (kLds ? part : g) + (id - 1) * PF_SEG_SUMS;
#pragma unroll
        for (int k = 0; k < PF_SEG_SUMS; ++k) {
            if (k < used && s[k] != 0) {
                if (kLds) __hip_atomic_fetch_add(dst + k, s[k], PF_SG_RLX_WG);
                else __hip_atomic_fetch_add(dst + k, s[k], PF_SG_RLX_AGENT);
            }
        }
    }
    if (kLds) {
        __syncthreads();
        for (int k = threadIdx.x; k < cells; k += kFlat) {
            const long long v = part[k];
            if (v != 0) __hip_atomic_fetch_add(g + k, v, PF_SG_RLX_AGENT);
        }
    }
}

__global__ void __launch_bounds__(64) pf_seg_objects_resolve(const PfSegObjArgs a) {
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k < a.M) pf_seg_resolve_object(a, (long)blockIdx.y, k);
}

int pf_sg_cus() {
    constexpr int MAX_DEV = 64;
    static int cus_of[MAX_DEV] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEV) dev = 0;
    if (cus_of[dev] == 0) {
        int n = 256;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cus_of[dev] = n;
    }
    return cus_of[dev];
}
unsigned pf_sg_blocks(long items, int per) { return (unsigned)((items + per - 1) / per); }
#define PF_SG_LAUNCHED() do { const int rl_ = (int)hipGetLastError(); if (rl_ != 0) return rl_; } while (0)
}  // namespace

extern "C" long pf_seg_scratch_bytes(int B, int H, int W) { return pf_seg_bytes(B, H, W); }

extern "C" int pf_seg_tables(float* rows, float* cols, int H, int W, void* stream) {
    const int rc = pf_seg_tables_check(rows, cols, H, W);
    if (rc != PF_OK) return rc;
    hipLaunchKernelGGL(pf_seg_tables_kernel, dim3(pf_sg_blocks((long)H + W, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, rows, cols, H, W);
    return (int)hipGetLastError();
}

extern "C" int pf_seg_label(const unsigned char* mask, const float* rows, int* labels, void* scratch, long scratch_bytes, int B, int H,
                            int W, int connectivity, int poles, void* stream) {
    PfSegLabelArgs a;
    const int rc = pf_seg_label_check(mask, rows, labels, scratch, scratch_bytes, B, H, W, connectivity, poles, a);
    if (rc != PF_OK) return rc;
    const hipStream_t st = (hipStream_t)stream;
    const long tiles = (long)((W + PF_SG_TW - 1) / PF_SG_TW) * ((H + PF_SG_TH - 1) / PF_SG_TH);     // < 2^30 / 2048 + H + W
    hipLaunchKernelGGL(pf_seg_label_local, dim3((unsigned)tiles, (unsigned)B), dim3(kBlock), 0, st, a);
    PF_SG_LAUNCHED();
    const long items = pf_seg_merge_items(H, W);                                                  // < 2^30 / 32 + 2^30 / 64 + H
    const unsigned item_blocks = pf_sg_blocks(items, kBlock);
    hipLaunchKernelGGL(pf_seg_label_merge, dim3(item_blocks + (poles ? 2u : 0u), (unsigned)B), dim3(kBlock), 0, st, a, items, item_blocks);
    PF_SG_LAUNCHED();
    hipLaunchKernelGGL(pf_seg_label_flatten, dim3(pf_sg_blocks((long)H * W, kFlat), (unsigned)B), dim3(kFlat), 0, st, a);
    return (int)hipGetLastError();
}

extern "C" int pf_seg_objects(const int* labels, const float* values, const float* rows, const float* cols, void* scratch,
                              long scratch_bytes, int* ids, unsigned char* keep, int* roots, int* count, float* table, void* sums, int B,
                              int C, int H, int W, int max_objects, float min_area, void* stream) {
    PfSegObjArgs a;
    const int rc = pf_seg_objects_check(labels, values, rows, cols, scratch, scratch_bytes, ids, keep, roots, count, table, sums, B, C, H,
                                        W, max_objects, min_area, a);
    if (rc != PF_OK) return rc;
    const hipStream_t st = (hipStream_t)stream;
    const dim3 row_grid(pf_sg_blocks(H, kWaves), (unsigned)B);
    hipLaunchKernelGGL(pf_seg_rank_count, row_grid, dim3(kBlock), 0, st, a);
    PF_SG_LAUNCHED();
    hipLaunchKernelGGL(pf_seg_rank_scan, dim3((unsigned)B), dim3(kBlock), 0, st, a);
    PF_SG_LAUNCHED();
    hipLaunchKernelGGL(pf_seg_rank_assign, row_grid, dim3(kBlock), 0, st, a);
    PF_SG_LAUNCHED();
    // two workgroups of 1024 per CU in all: every workgroup ends with one atomic per non-zero cell, and those of a large object
    // all meet on the same ten addresses
    const long want = pf_sg_blocks((long)H * W, kFlat), cap = (2L * pf_sg_cus() + B - 1) / B;
    const dim3 acc_grid((unsigned)(want < cap ? want : cap), (unsigned)B);
    if (max_objects <= kLdsObjects)
        hipLaunchKernelGGL(pf_seg_objects_accumulate<true>, acc_grid, dim3(kFlat), (size_t)max_objects * PF_SEG_SUMS * 8, st, a);
    else
        hipLaunchKernelGGL(pf_seg_objects_accumulate<false>, acc_grid, dim3(kFlat), 0, st, a);
    PF_SG_LAUNCHED();
    hipLaunchKernelGGL(pf_seg_objects_resolve, dim3(pf_sg_blocks(max_objects, 64), (unsigned)B), dim3(64), 0, st, a);
    return (int)hipGetLastError();
}

#ifdef PF_SG_STANDALONE                      // a library of this file alone (profiles/time_segments.py --lib)
extern "C" const char* pf_version(void) { return "priorflow segments, a build of its own"; }
#endif
