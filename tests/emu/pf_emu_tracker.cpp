// Host emulation of pf_trk_begin / pf_trk_vote / pf_trk_match / pf_trk_paint -- TEST INFRASTRUCTURE ONLY (its own library,
// libpf_emu_tracker.so).  The vote of a pixel, the admissible cells, the arg-max, the per-slot bookkeeping and the argument checks
// are prior-flow_amd/csrc/pf_tracker.h, the file the device kernels compile; a launch is restated as a loop over its grid, an
// atomic add as a plain one.  The product never loads this library.
//
// pf_emu_trk_order picks the order in which the vote loop visits the pixels of an image: 0 row by row, 1 reversed, any other value
// a fixed pseudo-random permutation seeded with it.  Integer adds commute, so the votes must not notice
// (tests/test_tracker_host.py).  The library also holds pf_emu_segments.cpp's entry points, so that one handle serves a
// MovingObjects and the ObjectTracker behind it.
#include "pf_tracker.h"
// the segment entry points, their visiting order (g_order, visit_order) and pf_version
#include "pf_emu_segments.cpp"

extern "C" void pf_emu_trk_order(unsigned long long seed) { g_order = seed; }

extern "C" int pf_trk_begin(void* votes, int B, int M, void*) {
    const int rc = pf_trk_begin_check(votes, B, M);
    if (rc != PF_OK) return rc;
    std::fill_n(static_cast<long long*>(votes), (long)B * M * M, 0LL);
    return PF_OK;
}

static void vote(const PfTrkVoteArgs& a) {
    const long N = (long)a.H * a.W;
    const std::vector<long> order = visit_order(N);
    for (long b = 0; b < a.B; ++b)
        for (long n : order) {
            const int y = (int)(n / a.W), x = (int)(n % a.W);
            const int cell = pf_trk_vote_cell(a, b, y, x);
            if (cell >= 0) a.S[b * a.M * a.M + cell] += pf_seg_area_q(a.rows[2 * y]);
        }
}

extern "C" int pf_trk_vote(const int* prev_ids, const int* ids, const float* flow_prev, const float* flow_cur,
                           const unsigned char* mask_prev, const unsigned char* mask_cur, const float* rows, void* votes, int B, int H,
                           int W, int M, void*) {
    PfTrkVoteArgs fwd, bwd;
    const int rc = pf_trk_vote_check(prev_ids, ids, flow_prev, flow_cur, mask_prev, mask_cur, rows, votes, B, H, W, M, fwd, bwd);
    if (rc != PF_OK) return rc;
    if (flow_prev) vote(fwd);
    if (flow_cur) vote(bwd);
    return PF_OK;
}

extern "C" int pf_trk_match(const void* votes, const int* count, const void* sums, int* st_count, void* st_sums, int* st_track,
                            int* st_age, float* st_path, int* next_id, int* track, int* age, int* origin, int* fate, float* step,
                            float* path, int B, int M, int n_dir, float min_overlap, void*) {
    PfTrkMatchArgs g;
    const int rc = pf_trk_match_check(votes, count, sums, st_count, st_sums, st_track, st_age, st_path, next_id, track, age, origin, fate,
                                      step, path, B, M, n_dir, min_overlap, g);
    if (rc != PF_OK) return rc;
    std::vector<long long> ap(M), ac(M), bear(3 * M);
    std::vector<int> ptrack(M), page(M), rowbest(M), colbest(M);
    std::vector<float> ppath(M);
    for (long b = 0; b < B; ++b) {
        const int n_c = pf_trk_rows(count[b], M);
        PfTrkPrev p;
        p.n_p = pf_trk_rows(st_count[b], M);
        p.next_id = next_id[b];
        for (int t = 0; t < M; ++t) {                                  // the previous state, before anything is written
            const long o = b * M + t;
            const long long* ps = g.st_sums + o * PF_SEG_SUMS;
            ap[t] = ps[0]; bear[3 * t] = ps[2]; bear[3 * t + 1] = ps[3]; bear[3 * t + 2] = ps[4];
            ac[t] = g.sums[o * PF_SEG_SUMS];
            ptrack[t] = st_track[o]; page[t] = st_age[o]; ppath[t] = st_path[o];
        }
        p.area = ap.data(); p.bear = bear.data(); p.track = ptrack.data(); p.age = page.data(); p.path = ppath.data();
        const long long* S = g.S + b * M * M;
        for (int t = 0; t < M; ++t) {
            rowbest[t] = t < p.n_p ? pf_trk_rowbest(S, t, n_c, M, ap.data(), ac.data(), n_dir, min_overlap) : -1;
            colbest[t] = t < n_c ? pf_trk_colbest(S, t, p.n_p, M, ap.data(), ac.data(), n_dir, min_overlap) : -1;
        }
        int fresh = 0;
        for (int t = 0; t < M; ++t) {
            pf_trk_slot(g, p, b, t, n_c, rowbest.data(), colbest.data(), fresh);
            fresh += pf_trk_is_new(t, n_c, rowbest.data(), colbest.data()) ? 1 : 0;
        }
        st_count[b] = count[b];
        next_id[b] = p.next_id + fresh;
    }
    return PF_OK;
}

extern "C" int pf_trk_paint(const int* ids, const int* track, int* track_map, int* st_ids, int B, int H, int W, int M, void*) {
    PfTrkPaintArgs a;
    const int rc = pf_trk_paint_check(ids, track, track_map, st_ids, B, H, W, M, a);
    if (rc != PF_OK) return rc;
    for (long b = 0; b < B; ++b)
        for (long n = 0; n < (long)H * W; ++n) pf_trk_paint_pixel(a, b, n);
    return PF_OK;
}
