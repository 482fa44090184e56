// Two choices of csrc/pf_egomotion.hip measured both ways, stand-alone:
//
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fno-slp-vectorize -I prior-flow_amd/csrc profiles/ego_variants.hip -o profiles/scratch/ego_variants
//   profiles/scratch/ego_variants [H W]          (default 512 1024, B = 1; prints one JSON line)
//
//   (1) passes >= 1 of pf_ego_accumulate: RECOMPUTE p and q from the flow (what ships: 8 bytes and six transcendentals per pixel)
//       against reading q back from a SCRATCH PLANE that pass 0 wrote (12 bytes and two transcendentals per pixel in the later
//       passes, 12 bytes more written in pass 0; a left-out pixel is a NaN in the plane, so the later passes read neither flow nor
//       mask).
//   (2) pf_erp_rotate: ONE output pixel per thread (what ships) against 2 and 4 pixels of one row per thread, which share the
//       row's sin phi, cos phi and the loads of R.
// The shipped kernels are the ones of the library (the unit is included as it is); the variants differ only in what is named
// above.  Each figure is microseconds per launch over back-to-back launches between two events, the median of nine rounds.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pf_egomotion.hip"

#define CK(call) do { if ((call) != hipSuccess) { fprintf(stderr, "HIP error at line %d\n", __LINE__); exit(6); } } while (0)

namespace {
// (1) the scratch-plane variant of pf_ego_acc_kernel: MODE 0 = pass 0 (computes and stores q), MODE 1 = a later pass (loads q)
template <int MODE>
__global__ void __launch_bounds__(kAccBlock) acc_plane_kernel(const PfEgoAccArgs a, float* plane) {
    __shared__ long long part[kWaves][PF_EGO_SUMS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y;
    const long N = (long)a.H * a.W;
    float R[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = a.R[b * 9 + k];
    const float* fu = a.flow + (long)b * 2 * N;
    const float* fv = fu + N;
    float* pl = plane + (long)b * 3 * N;
    long long s[PF_EGO_SUMS];
#pragma unroll
    for (int k = 0; k < PF_EGO_SUMS; ++k) s[k] = 0;
    const int per_row = (a.W + kStrip * 64 - 1) / (kStrip * 64);
    const long strips = (long)a.H * per_row;
    for (long i = (long)blockIdx.x * kWaves + wave; i < strips; i += (long)gridDim.x * kWaves) {
        const int y = (int)(i / per_row), x0 = (int)(i - (long)y * per_row) * (kStrip * 64) + lane;
        float cp, sp;
        pf_ego_row(y, a.H, cp, sp);
        for (int k = 0; k < kStrip; ++k) {
            const int x = x0 + k * 64;
            if (x >= a.W) break;
            const long n = (long)y * a.W + x;
            PfVec3 q;
            if (MODE == 0) {
                const float u = fu[n], v = fv[n];
                const bool out = pf_ego_left_out(u, v, 0);
                q = pf_ego_q(x, y, out ? 0.f : u, out ? 0.f : v, a.H, a.W);
                if (out) q.x = __builtin_nanf("");
                pl[n] = q.x; pl[N + n] = q.y; pl[2 * N + n] = q.z;
            } else {
                q.x = pl[n]; q.y = pl[N + n]; q.z = pl[2 * N + n];
            }
            if (q.x != q.x) continue;
            const PfVec3 p = pf_ego_p(x, a.W, cp, sp);
            const float r2 = pf_ego_chord2(R, p, q);
            float w = cp;
            if (a.weighted) {
                const float t = 1.f + r2 * a.inv_c2;
                w = cp * (1.f / (t * t));
            }
            const float wx = w * p.x, wy = w * p.y, wz = w * p.z;
            s[0] += pf_ego_quant(wx * q.x, a.f); s[1] += pf_ego_quant(wx * q.y, a.f); s[2] += pf_ego_quant(wx * q.z, a.f);
            s[3] += pf_ego_quant(wy * q.x, a.f); s[4] += pf_ego_quant(wy * q.y, a.f); s[5] += pf_ego_quant(wy * q.z, a.f);
            s[6] += pf_ego_quant(wz * q.x, a.f); s[7] += pf_ego_quant(wz * q.y, a.f); s[8] += pf_ego_quant(wz * q.z, a.f);
            s[9] += pf_ego_quant(w, a.f);
            s[10] += pf_ego_quant(w * r2, a.fr);
            s[11] += 1;
        }
    }
#pragma unroll
    for (int k = 0; k < PF_EGO_SUMS; ++k) {
        long long v = s[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if (lane == 0) part[wave][k] = v;
    }
    __syncthreads();
    if (tid < PF_EGO_SUMS) {
        long long v = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) v += part[w][tid];
        if (v != 0) atomicAdd(reinterpret_cast<unsigned long long*>(a.sums + (long)b * PF_EGO_SUMS + tid), (unsigned long long)v);
    }
}
// (2) PPT pixels of one row per thread: grid (ceil(W / (256 PPT)), H, B)
template <int PPT>
__global__ void __launch_bounds__(kBlock) rotate_row_kernel(const PfErpRotArgs a) {
    const int y = blockIdx.y, b = blockIdx.z;
    float R[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = a.R[b * 9 + k];
    float cp, sp;
    pf_ego_row(y, a.H, cp, sp);
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const int x = ((int)blockIdx.x * PPT + k) * kBlock + (int)threadIdx.x;
        if (x < a.W) pf_erp_rotate_pixel(a, R, b, y, x, cp, sp);
    }
}

template <class F>
double time_us(F launch, int n) {
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    std::vector<double> rounds;
    for (int r = 0; r < 9; ++r) {
        for (int i = 0; i < 10; ++i) launch();
        CK(hipEventRecord(e0, 0));
        for (int i = 0; i < n; ++i) launch();
        CK(hipEventRecord(e1, 0));
        CK(hipEventSynchronize(e1));
        float ms = 0.f;
        CK(hipEventElapsedTime(&ms, e0, e1));
        rounds.push_back(1000.0 * ms / n);
    }
    std::sort(rounds.begin(), rounds.end());
    return rounds[rounds.size() / 2];
}
}  // namespace

int main(int argc, char** argv) {
    const int H = argc > 2 ? atoi(argv[1]) : 512, W = argc > 2 ? atoi(argv[2]) : 1024, B = 1, C = 3, n = 200;
    const long N = (long)H * W;
    if (H < 1 || W < 1 || N >= (1L << 28)) return 2;
    std::vector<float> flow(2 * N), frame(C * N);
    for (long i = 0; i < N; ++i) {
        const int y = (int)(i / W), x = (int)(i % W);
        flow[i] = 5.f + 3.f * sinf(0.01f * (float)x) + ((i * 2654435761u) % 1000) * 1e-4f;
        flow[N + i] = 2.f * cosf(0.02f * (float)y);
        for (int c = 0; c < C; ++c) frame[c * N + i] = (float)((i * 40503u + c * 977u) % 256);
    }
    const float Rh[9] = {0.9990482f, -0.0432f, 0.0058f, 0.0433f, 0.9989f, -0.0174f, -0.0050f, 0.0176f, 0.9998f};
    float *d_flow, *d_frame, *d_out, *d_plane, *d_R;
    long long* d_sums;
    CK(hipMalloc(&d_flow, 2 * N * 4)); CK(hipMalloc(&d_frame, C * N * 4)); CK(hipMalloc(&d_out, C * N * 4)); CK(hipMalloc(&d_plane, 3 * N * 4));
    CK(hipMalloc(&d_R, 9 * 4)); CK(hipMalloc(&d_sums, PF_EGO_SUMS * 8));
    CK(hipMemcpy(d_flow, flow.data(), 2 * N * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_frame, frame.data(), C * N * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_R, Rh, 9 * 4, hipMemcpyHostToDevice));
    CK(hipMemset(d_sums, 0, PF_EGO_SUMS * 8));
    PfEgoAccArgs a;
    if (pf_ego_accumulate_check(d_flow, nullptr, d_R, d_sums, B, H, W, 1, 1.f, 0, a) != PF_OK) return 3;
    PfEgoAccArgs a0 = a;
    a0.weighted = 0;
    const long strips = (long)H * ((W + kStrip * 64 - 1) / (kStrip * 64));
    const long need = (strips + kWaves - 1) / kWaves;
    const unsigned bx = (unsigned)std::max(1L, std::min(need, (long)pf_ego_cus()));
    const dim3 grid(bx, B);
    long long ref[PF_EGO_SUMS], got[PF_EGO_SUMS];
    hipLaunchKernelGGL(pf_ego_acc_kernel, grid, dim3(kAccBlock), 0, 0, a);
    CK(hipMemcpy(ref, d_sums, sizeof ref, hipMemcpyDeviceToHost));
    CK(hipMemset(d_sums, 0, PF_EGO_SUMS * 8));
    hipLaunchKernelGGL(acc_plane_kernel<0>, grid, dim3(kAccBlock), 0, 0, a0, d_plane);
    CK(hipMemset(d_sums, 0, PF_EGO_SUMS * 8));
    hipLaunchKernelGGL(acc_plane_kernel<1>, grid, dim3(kAccBlock), 0, 0, a, d_plane);
    CK(hipMemcpy(got, d_sums, sizeof got, hipMemcpyDeviceToHost));
    bool same = true;
    for (int k = 0; k < PF_EGO_SUMS; ++k) same = same && ref[k] == got[k];
    const double t_re0 = time_us([&] { hipLaunchKernelGGL(pf_ego_acc_kernel, grid, dim3(kAccBlock), 0, 0, a0); }, n);
    const double t_re1 = time_us([&] { hipLaunchKernelGGL(pf_ego_acc_kernel, grid, dim3(kAccBlock), 0, 0, a); }, n);
    const double t_pl0 = time_us([&] { hipLaunchKernelGGL(acc_plane_kernel<0>, grid, dim3(kAccBlock), 0, 0, a0, d_plane); }, n);
    const double t_pl1 = time_us([&] { hipLaunchKernelGGL(acc_plane_kernel<1>, grid, dim3(kAccBlock), 0, 0, a, d_plane); }, n);
    PfErpRotArgs r;
    if (pf_erp_rotate_check(d_frame, d_out, d_R, B, C, H, W, PF_VIEW_F32, r) != PF_OK) return 4;
    const double t_r1 = time_us([&] { hipLaunchKernelGGL(pf_erp_rotate_kernel, dim3(pf_ego_blocks(N), B), dim3(kBlock), 0, 0, r); }, n);
    const double t_r1r = time_us([&] { hipLaunchKernelGGL(rotate_row_kernel<1>, dim3((W + kBlock - 1) / kBlock, H, B), dim3(kBlock), 0, 0, r); }, n);
    const double t_r2 = time_us([&] { hipLaunchKernelGGL(rotate_row_kernel<2>, dim3((W + 2 * kBlock - 1) / (2 * kBlock), H, B), dim3(kBlock), 0, 0, r); }, n);
    const double t_r4 = time_us([&] { hipLaunchKernelGGL(rotate_row_kernel<4>, dim3((W + 4 * kBlock - 1) / (4 * kBlock), H, B), dim3(kBlock), 0, 0, r); }, n);
    if (hipDeviceSynchronize() != hipSuccess) return 5;
    printf("{\"shape\": [%d, %d], \"launches_per_figure\": %d, \"plane_sums_equal_recompute\": %s, "
           "\"accumulate_us\": {\"recompute_plain\": %.2f, \"recompute_weighted\": %.2f, \"plane_pass0\": %.2f, \"plane_later\": %.2f}, "
           "\"estimate_of_4_passes_us\": {\"recompute\": %.2f, \"plane\": %.2f}, "
           "\"rotate_f32_us\": {\"one_pixel_shipped\": %.2f, \"row_1\": %.2f, \"row_2\": %.2f, \"row_4\": %.2f}}\n",
           H, W, n, same ? "true" : "false", t_re0, t_re1, t_pl0, t_pl1, t_re0 + 3 * t_re1, t_pl0 + 3 * t_pl1, t_r1, t_r1r, t_r2, t_r4);
    return 0;
}
