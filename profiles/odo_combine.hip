// The OTHER form of pf_odo_accumulate (prior-flow_amd/csrc/pf_odometry.hip), kept for its measurement only:
// the library's kernel lets every lane add to the LDS histogram alone; this one combines inside the wave first.  Up to two times
// the lowest active lane names its bin, the lanes that share it add up their two contributions with cross-lane moves and ONE lane
// makes the two LDS adds; a second round runs only when the first took at least half of the lanes, and whoever is left adds
// alone.  Integer adds commute, so the cells are the library's bit for bit.  Measured at 512 x 1024, 512 bins
// (profiles/r14_odometry_time.json): 14.2 us on a concentrated input and 17.0 us on a spread one, against 14.6 and 15.5 us of the
// library's form, which was kept.
//
// A library of its own with pf_odo_accumulate (and pf_odo_hist_bytes, pf_version) only, for `time_odometry.py --lib`:
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fno-slp-vectorize -fPIC -shared -I prior-flow_amd/csrc \
//         profiles/odo_combine.hip -o profiles/scratch/libpf_odometry_combine.so
#include "pf_odometry.h"

namespace {
constexpr int kAccBlock = 1024, kWaves = kAccBlock / 64;
constexpr int kStrip = 2;
constexpr int kRounds = 2;

__device__ inline long long wave_sum(long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}
__device__ inline void lds_add(unsigned long long* cell, long long v) { atomicAdd(cell, (unsigned long long)v); }

template <int ROUNDS>
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
            bool mine = ok;                                              // still to be added
            if (ROUNDS > 0) {
                unsigned long long left = __ballot(mine);
#pragma unroll
                for (int r = 0; r < ROUNDS; ++r) {
                    if (left == 0) break;                               // wave-uniform
                    const int lead = __ffsll((long long)left) - 1;
                    const int b0 = __shfl(bin, lead, 64);
                    const bool same = mine && bin == b0;
                    const unsigned long long took = __ballot(same);
                    const long long sw = wave_sum(same ? qw : 0), sm = wave_sum(same ? qm : 0);
                    if (lane == 0) { lds_add(&hist[b0], sw); lds_add(&hist[bins + b0], sm); }
                    mine = mine && !same;
                    const int had = __popcll(left);
                    left &= ~took;
                    if (2 * __popcll(took) < had) break;                // spread bins: the rest goes lane by lane
                }
            }
            if (mine) { lds_add(&hist[bin], qw); lds_add(&hist[bins + bin], qm); }
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
    hipLaunchKernelGGL(pf_odo_acc_kernel<kRounds>, dim3((unsigned)bx, (unsigned)B), dim3(kAccBlock), (size_t)2 * bins * 8,
                       (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

extern "C" const char* pf_version(void) { return "profiles/odo_combine.hip: pf_odo_accumulate combining inside the wave (gfx950)"; }
