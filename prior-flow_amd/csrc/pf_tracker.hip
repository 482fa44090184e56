// Object tracks on the device: the statement is pf_tracker.h.  Everything runs on the stream it is given,
// reads nothing on the host and allocates nothing.  A push is four launches with one flow, five with two; no memset.
//
//   pf_trk_begin_kernel   one thread per cell of votes: zero.
//   pf_trk_vote_kernel    one launch per flow; a grid sized by the CU count (1024 threads, two workgroups per CU in all).  A wave
//     takes 64 consecutive pixels of one row: the id, u, v and mask reads are coalesced, the id at the target is one gather.  Every
//     lane of the wave has the same weight (cos phi of the row), so the lanes that share a cell (a, b) are counted with a ballot
//     and go out as ONE atomic of count * weight per distinct cell of the wave.  M <= 64: the partial matrix lives in LDS as
//     64-bit integers (8 M M bytes, 32 KiB at M = 64) and leaves with one global 64-bit atomic per non-zero cell; a larger M goes
//     straight to global atomics.
//   pf_trk_match_kernel   one workgroup of 256 per image, thread t = slot t: the previous state into LDS, a barrier, the row and
//     column arg-max, a barrier, a scan over the new slots, every [B,M] output and the state of the next push.
//   pf_trk_paint_kernel   one thread per pixel.
//
// Every index is a pixel below H * W, an image below B, a slot below M or a cell below M * M; an id is compared with 1..M before it
// indexes anything (pf_trk_vote_cell, pf_trk_paint_pixel), a count is clamped to 0..M (pf_trk_rows).
#include "pf_tracker.h"

namespace {
constexpr int kBlock = 256;
constexpr int kVote = 1024, kVoteWaves = kVote / 64;

#define PF_TK_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT
#define PF_TK_RLX_WG __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP

__global__ void __launch_bounds__(kBlock) pf_trk_begin_kernel(long long* S, long cells) {
    const long i = (long)blockIdx.x * kBlock + threadIdx.x;
    if (i < cells) S[i] = 0;
}

template <bool kLds>
__global__ void __launch_bounds__(kVote) pf_trk_vote_kernel(const PfTrkVoteArgs a) {
    extern __shared__ long long part[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, cells = a.M * a.M;
    const long b = blockIdx.y;
    long long* g = a.S + b * cells;
    if (kLds) {
        for (int k = threadIdx.x; k < cells; k += kVote) part[k] = 0;
        __syncthreads();
    }
    const int segs = (a.W + 63) / 64;
    const long items = (long)a.H * segs;
    for (long it = (long)blockIdx.x * kVoteWaves + wave; it < items; it += (long)gridDim.x * kVoteWaves) {       // the same for a whole wave
        const int y = (int)(it / segs), x = (int)(it - (long)y * segs) * 64 + lane;
        const int key = x < a.W ? pf_trk_vote_cell(a, b, y, x) : -1;
        unsigned long long todo = __ballot(key >= 0);
        if (!todo) continue;
        const long long q = pf_seg_area_q(a.rows[2 * y]);
        while (todo) {                                            // one turn per distinct cell of the wave
            const int first = __ffsll((long long)todo) - 1;
            const int k0 = __shfl(key, first);
            const unsigned long long same = __ballot(key == k0);
            if (lane == first && q != 0) {
                const long long s = q * __popcll(same);
                if (kLds) __hip_atomic_fetch_add(part + k0, s, PF_TK_RLX_WG);
                else __hip_atomic_fetch_add(g + k0, s, PF_TK_RLX_AGENT);
            }
            todo &= ~same;
        }
    }
    if (kLds) {
        __syncthreads();
        for (int k = threadIdx.x; k < cells; k += kVote) {
            const long long v = part[k];
            if (v != 0) __hip_atomic_fetch_add(g + k, v, PF_TK_RLX_AGENT);
        }
    }
}

__global__ void __launch_bounds__(kBlock) pf_trk_match_kernel(const PfTrkMatchArgs g) {
    __shared__ long long ap[kBlock], ac[kBlock], bear[3 * kBlock];
    __shared__ int ptrack[kBlock], page[kBlock], rowbest[kBlock], colbest[kBlock], scan[kBlock];
    __shared__ float ppath[kBlock];
    const int t = threadIdx.x, M = g.M;
    const long b = blockIdx.x, o = b * M + t;
    const int count = g.count[b], n_c = pf_trk_rows(count, M);
    PfTrkPrev p;
    p.n_p = pf_trk_rows(g.st_count[b], M);
    p.next_id = g.next_id[b];
    p.area = ap; p.bear = bear; p.track = ptrack; p.age = page; p.path = ppath;
    if (t < M) {
        const long long* ps = g.st_sums + o * PF_SEG_SUMS;
        ap[t] = ps[0]; bear[3 * t] = ps[2]; bear[3 * t + 1] = ps[3]; bear[3 * t + 2] = ps[4];
        ac[t] = g.sums[o * PF_SEG_SUMS];
        ptrack[t] = g.st_track[o]; page[t] = g.st_age[o]; ppath[t] = g.st_path[o];
    }
    __syncthreads();                                              // everything previous has been read: the state may be written
    const long long* S = g.S + b * M * M;
    rowbest[t] = t < p.n_p ? pf_trk_rowbest(S, t, n_c, M, ap, ac, g.n_dir, g.min_overlap) : -1;
    colbest[t] = t < n_c ? pf_trk_colbest(S, t, p.n_p, M, ap, ac, g.n_dir, g.min_overlap) : -1;
    __syncthreads();
    const int fresh = pf_trk_is_new(t, n_c, rowbest, colbest) ? 1 : 0;
    scan[t] = fresh;
    __syncthreads();
    for (int d = 1; d < kBlock; d <<= 1) {
        const int v = t >= d ? scan[t - d] : 0;
        __syncthreads();
        scan[t] += v;
        __syncthreads();
    }
    if (t < M) pf_trk_slot(g, p, b, t, n_c, rowbest, colbest, scan[t] - fresh);
    if (t == 0) { g.st_count[b] = count; g.next_id[b] = p.next_id + scan[kBlock - 1]; }
}

__global__ void __launch_bounds__(kBlock) pf_trk_paint_kernel(const PfTrkPaintArgs a) {
    const long n = (long)blockIdx.x * kBlock + threadIdx.x;
    if (n < (long)a.H * a.W) pf_trk_paint_pixel(a, (long)blockIdx.y, n);
}

int pf_tk_cus() {
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
unsigned pf_tk_blocks(long items, int per) { return (unsigned)((items + per - 1) / per); }

int pf_tk_launch_vote(const PfTrkVoteArgs& a, hipStream_t st) {
    // few large workgroups, as pf_seg_objects_accumulate: every workgroup ends on the same few cells
    const long items = (long)a.H * ((a.W + 63) / 64);
    const long want = pf_tk_blocks(items, kVoteWaves), cap = (2L * pf_tk_cus() + a.B - 1) / a.B;
    const dim3 grid((unsigned)(want < cap ? want : cap), (unsigned)a.B);
    if (a.M <= PF_TK_LDS_OBJECTS)
        hipLaunchKernelGGL(pf_trk_vote_kernel<true>, grid, dim3(kVote), (size_t)a.M * a.M * 8, st, a);
    else
        hipLaunchKernelGGL(pf_trk_vote_kernel<false>, grid, dim3(kVote), 0, st, a);
    return (int)hipGetLastError();
}
}  // namespace

extern "C" int pf_trk_begin(void* votes, int B, int M, void* stream) {
    const int rc = pf_trk_begin_check(votes, B, M);
    if (rc != PF_OK) return rc;
    const long cells = (long)B * M * M;                           // <= 65535 * 2^16
    hipLaunchKernelGGL(pf_trk_begin_kernel, dim3(pf_tk_blocks(cells, kBlock)), dim3(kBlock), 0, (hipStream_t)stream,
                       static_cast<long long*>(votes), cells);
    return (int)hipGetLastError();
}

extern "C" int pf_trk_vote(const int* prev_ids, const int* ids, const float* flow_prev, const float* flow_cur,
                           const unsigned char* mask_prev, const unsigned char* mask_cur, const float* rows, void* votes, int B, int H,
                           int W, int M, void* stream) {
    PfTrkVoteArgs fwd, bwd;
    const int rc = pf_trk_vote_check(prev_ids, ids, flow_prev, flow_cur, mask_prev, mask_cur, rows, votes, B, H, W, M, fwd, bwd);
    if (rc != PF_OK) return rc;
    if (flow_prev) {
        const int rl = pf_tk_launch_vote(fwd, (hipStream_t)stream);
        if (rl != 0) return rl;
    }
    return flow_cur ? pf_tk_launch_vote(bwd, (hipStream_t)stream) : PF_OK;
}

extern "C" int pf_trk_match(const void* votes, const int* count, const void* sums, int* st_count, void* st_sums, int* st_track,
                            int* st_age, float* st_path, int* next_id, int* track, int* age, int* origin, int* fate, float* step,
                            float* path, int B, int M, int n_dir, float min_overlap, void* stream) {
    PfTrkMatchArgs a;
    const int rc = pf_trk_match_check(votes, count, sums, st_count, st_sums, st_track, st_age, st_path, next_id, track, age, origin, fate,
                                      step, path, B, M, n_dir, min_overlap, a);
    if (rc != PF_OK) return rc;
    hipLaunchKernelGGL(pf_trk_match_kernel, dim3((unsigned)B), dim3(kBlock), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

extern "C" int pf_trk_paint(const int* ids, const int* track, int* track_map, int* st_ids, int B, int H, int W, int M, void* stream) {
    PfTrkPaintArgs a;
    const int rc = pf_trk_paint_check(ids, track, track_map, st_ids, B, H, W, M, a);
    if (rc != PF_OK) return rc;
    hipLaunchKernelGGL(pf_trk_paint_kernel, dim3(pf_tk_blocks((long)H * W, kBlock), (unsigned)B), dim3(kBlock), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}
