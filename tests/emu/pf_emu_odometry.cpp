// Host emulation of pf_odo_accumulate / pf_odo_solve / pf_odo_reverse_pose / pf_odo_track / pf_odo_fuse -- TEST INFRASTRUCTURE
// ONLY (its own library, libpf_emu_odometry.so).  The per-pixel and per-image arithmetic, the scales and the argument checks are
// prior-flow_amd/csrc/pf_odometry.h, the file the device kernels compile; a launch is restated as a loop over its grid, an atomic
// add as a plain add.  The product never loads this library.
//
// pf_emu_odo_order picks the order in which the accumulate loop visits the pixels of an image: 0 row by row, 1 reversed, any
// other value a fixed pseudo-random permutation seeded with it.  Integer adds commute, so the cells must not notice
// (tests/test_odometry_host.py).  The library also holds pf_emu_epipolar.cpp's entry points, so that one handle serves a whole Odometry.
#include "pf_odometry.h"
// the pose entry points an Odometry needs beside its own, their visiting order (g_order, visit_order) and pf_version
#include "pf_emu_epipolar.cpp"

extern "C" void pf_emu_odo_order(unsigned long long seed) { g_order = seed; }

extern "C" long pf_odo_hist_bytes(int B, int H, int W, int bins) { return pf_odo_bytes(B, H, W, bins); }

extern "C" int pf_odo_accumulate(const float* inv_a, const float* conf_a, const unsigned char* moving_a, const float* inv_b,
                                 const float* conf_b, const unsigned char* moving_b, void* hist, int B, int H, int W, int bins,
                                 float log2_range, float kappa_min, int blocks, void*) {
    PfOdoAccArgs a;
    const int rc = pf_odo_accumulate_check(inv_a, conf_a, moving_a, inv_b, conf_b, moving_b, hist, B, H, W, bins, log2_range, kappa_min,
                                           blocks, a);
    if (rc != PF_OK) return rc;
    const long N = (long)H * W;
    const std::vector<long> order = visit_order(N);
    for (long b = 0; b < B; ++b) {
        long long* h = a.hist + b * PF_ODO_CELLS(bins);
        for (long n : order) {
            const int y = (int)(n / W);
            float cp, sp;
            pf_ego_row(y, H, cp, sp);
            const long o = b * N + n;
            int bin;
            float w, lc;
            if (!pf_odo_link_pixel(a, cp, inv_a[o], conf_a[o], moving_a[o], inv_b[o], conf_b[o], moving_b[o], bin, w, lc)) continue;
            const long long qw = pf_odo_qw(a, w);
            h[bin] += qw; h[bins + bin] += pf_odo_qm(a, w, lc); h[2 * bins] += qw; h[2 * bins + 1] += 1;
        }
    }
    return PF_OK;
}

extern "C" int pf_odo_solve(void* hist, float* ratio, float* stats, int B, int H, int W, int bins, float log2_range, int trim_bins,
                            float min_used, float max_iqr, void*) {
    PfOdoSolveArgs a;
    const int rc = pf_odo_solve_check(hist, ratio, stats, B, H, W, bins, log2_range, trim_bins, min_used, max_iqr, a);
    if (rc != PF_OK) return rc;
    for (int b = 0; b < B; ++b) pf_odo_solve_image(a, b);
    return PF_OK;
}

extern "C" int pf_odo_reverse_pose(const float* R, const float* t, float* R_rev, float* t_rev, int B, void*) {
    PfOdoReverseArgs a;
    const int rc = pf_odo_reverse_check(R, t, R_rev, t_rev, B, a);
    if (rc != PF_OK) return rc;
    for (int b = 0; b < B; ++b) pf_odo_reverse_image(a, b);
    return PF_OK;
}

extern "C" int pf_odo_track(const float* R, const float* t, const float* pose_stats, const float* ratio, const float* link_stats,
                            void* state, float* orient, float* centre, float* baseline, int* flags, int B, void*) {
    PfOdoTrackArgs a;
    const int rc = pf_odo_track_check(R, t, pose_stats, ratio, link_stats, state, orient, centre, baseline, flags, B, a);
    if (rc != PF_OK) return rc;
    for (int b = 0; b < B; ++b) pf_odo_track_image(a, b);
    return PF_OK;
}

extern "C" int pf_odo_fuse(const float* inv_a, const float* conf_a, const unsigned char* moving_a, const float* inv_b, const float* conf_b,
                           const unsigned char* moving_b, const float* S_a, const float* S_b, const float* link_valid, float* inv_depth,
                           float* weight, unsigned char* disagree, int B, int H, int W, float conf_min, float kappa_min, float tol_log2,
                           void*) {
    PfOdoFuseArgs a;
    const int rc = pf_odo_fuse_check(inv_a, conf_a, moving_a, inv_b, conf_b, moving_b, S_a, S_b, link_valid, inv_depth, weight, disagree,
                                     B, H, W, conf_min, kappa_min, tol_log2, a);
    if (rc != PF_OK) return rc;
    for (int b = 0; b < B; ++b)
        for (long n = 0; n < (long)H * W; ++n) pf_odo_fuse_pixel(a, b, n);
    return PF_OK;
}

// the worst-case row of the overflow argument: every pixel of an H x W image adds the largest contribution (w = 1, l_c = L) to ONE
// bin, through the statement's quantisers; out = {W cell, M cell}
extern "C" void pf_emu_odo_worst(int H, int W, long long* out) {
    PfOdoAccArgs a;
    a.L = 4.f; a.f = pf_ego_scales(H, W).f;
    long long w = 0, m = 0;
    for (long i = 0; i < (long)H * W; ++i) { w += pf_odo_qw(a, 1.f); m += pf_odo_qm(a, 1.f, a.L); }
    out[0] = w; out[1] = m;
}
// cos phi of every row as the emulation's pf_ego_row gives it (section 19's code, which this library only calls)
extern "C" void pf_emu_odo_rows(int H, float* cp) {
    for (int y = 0; y < H; ++y) { float s; pf_ego_row(y, H, cp[y], s); }
}
