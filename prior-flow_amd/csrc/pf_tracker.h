// Object tracks: persistent ids for the objects of pf_seg_objects across frames, from flow votes (DESIGN.md section 26;
// include/priorflow_hip.h: pf_trk_begin, pf_trk_vote, pf_trk_match, pf_trk_paint).  The statement, once, for the device kernels
// (pf_tracker.hip), the host emulation (tests/emu/pf_emu_tracker.cpp) and the C checks.  The quantiser, the left-out rule and the
// area weight are pf_egomotion.h's and pf_segments.h's; nothing of them is restated here.
//
// Two object maps take part: the PREVIOUS one (ids, count, sums as the tracker kept them from the last push) and the CURRENT one
// (pf_seg_objects' outputs), both with M = max_objects rows; n_p = min(prev count, M), n_c = min(count, M) (a negative count: 0).
//
// Votes S int64 [B,M,M].  One or two flows vote: one on the previous grid pointing into the current frame, one on the current
// grid pointing into the previous frame.  Every source pixel (x, y) with a source id s in 1..M votes once.  Target:
// xt = floorf(((float)x + u) + 0.5f), yt = floorf(((float)y + v) + 0.5f) (adds only, each rounded once), xt wrapped into [0, W).
// Left out: mask byte non-zero, |u| or |v| not below 2^30 (pf_ego_left_out), yt outside [0, H).  With d the id at the target in the
// other map, 1 <= d <= M, the pixel adds pf_seg_area_q(rows[y].cos) to S[prev id - 1][cur id - 1]: the backward flow votes into
// the transposed cell.  A direction adds less than 2^30 2^32 = 2^62 to a cell, both less than 2^63.
//
// Admissible cells.  n_dir = the number of flows that voted, A_p, A_c the area sums (sums[..., 0]):
//   thr(a, b) = (int64) ceil((double)min_overlap * (double)(n_dir * min(A_p[a], A_c[b]))),
//   E[a][b] = S[a][b] when S[a][b] >= max(1, thr), else 0, for a < n_p and b < n_c.
// Match.  rowbest(a) = the smallest b that maximises E[a][.], -1 for an all-zero row; colbest(b) likewise.  A track continues from
// a to b when rowbest(a) = b and colbest(b) = a.
//
// Per current slot b < n_c (rows >= n_c are zero):
//   track   continued: the previous track of a; otherwise next_id + the number of new slots below b (next_id starts at 1 and
//           advances by the number of new slots)
//   age     previous age + 1 / 1            origin   the track itself / the track of colbest(b) when there is one (split) / 0
//   step    the great-circle angle between the previous and the current summed bearing (sums[..., 2:5]) in fp64:
//           atan2(|p x c|, p . c), rounded once to fp32; 0 for a new track or a vanishing bearing
//   path    previous path + step (one fp32 add) / 0
// Per previous slot a < n_p: fate = b + 1 continued, -(rowbest(a) + 1) when that slot went to another track (merged), 0 lost.
// track_map [B,H,W]: the track of each pixel's object, 0 where ids is 0.  After a push the state holds count, sums, track, age,
// path and ids of the current frame.  No address depends on an id that was not compared with M first.
#pragma once
#include "pf_segments.h"

static_assert(PF_TRK_MAX_OBJECTS == 256, "the sizes of pf_tracker.h and of the public header");
#define PF_TK_LDS_OBJECTS 64                 // M up to which the vote kernel keeps its partial matrix in LDS (32 KB)

struct PfTrkVoteArgs {
    const int* src; const int* dst; const float* flow; const unsigned char* mask; const float* rows;   // maps [B,H,W], flow [B,2,H,W]
    long long* S;                                                                                       // [B,M,M]
    int B, H, W, M, transposed;                                                                         // transposed: src is the current map
};
struct PfTrkMatchArgs {
    const long long* S; const int* count; const long long* sums;                                         // the current frame
    int* st_count; long long* st_sums; int* st_track; int* st_age; float* st_path; int* next_id;        // the state, in place
    int* track; int* age; int* origin; int* fate; float* step; float* path;                             // outputs [B,M]
    int B, M, n_dir; float min_overlap;
};
struct PfTrkPaintArgs { const int* ids; const int* track; int* track_map; int* st_ids; int B, H, W, M; };

PF_HD int pf_trk_rows(int count, int M) { return count < 0 ? 0 : (count < M ? count : M); }

// the cell a M + b that pixel (x, y) of image b votes into, or -1
PF_HD int pf_trk_vote_cell(const PfTrkVoteArgs& a, long b, int y, int x) {
    const long N = (long)a.H * a.W, n = (long)y * a.W + x;
    const int s = a.src[b * N + n];
    if (s <= 0 || s > a.M) return -1;
    const float u = a.flow[b * 2 * N + n], v = a.flow[(b * 2 + 1) * N + n];
    if (pf_ego_left_out(u, v, a.mask ? a.mask[b * N + n] : (unsigned char)0)) return -1;
    const float fx = floorf(((float)x + u) + 0.5f), fy = floorf(((float)y + v) + 0.5f);      // |fx|, |fy| <= 2^31: whole numbers
    if (!(fy >= 0.f && fy < PF_EGO_FAR)) return -1;
    const long long yt = (long long)fy;
    if (yt >= a.H) return -1;
    long long xt = (long long)fx % a.W;
    if (xt < 0) xt += a.W;
    const int d = a.dst[b * N + yt * a.W + xt];
    if (d <= 0 || d > a.M) return -1;
    return a.transposed ? (d - 1) * a.M + (s - 1) : (s - 1) * a.M + (d - 1);
}

// E[a][b] of S[a][b] = s under the two area sums
PF_HD long long pf_trk_admit(long long s, long long ap, long long ac, int n_dir, float min_overlap) {
    const long long m = ap < ac ? ap : ac;
    const long long thr = (long long)ceil((double)min_overlap * (double)((long long)n_dir * m));
    return s >= (thr > 1 ? thr : 1) ? s : 0;
}
// S: image b's matrix; ap [M], ac [M]: the area sums of the two frames
PF_HD int pf_trk_rowbest(const long long* S, int a, int n_c, int M, const long long* ap, const long long* ac, int n_dir, float mo) {
    long long best = 0;
    int at = -1;
    for (int b = 0; b < n_c; ++b) {
        const long long e = pf_trk_admit(S[(long)a * M + b], ap[a], ac[b], n_dir, mo);
        if (e > best) { best = e; at = b; }                      // strictly: ties stay with the smallest index
    }
    return at;
}
PF_HD int pf_trk_colbest(const long long* S, int b, int n_p, int M, const long long* ap, const long long* ac, int n_dir, float mo) {
    long long best = 0;
    int at = -1;
    for (int a = 0; a < n_p; ++a) {
        const long long e = pf_trk_admit(S[(long)a * M + b], ap[a], ac[b], n_dir, mo);
        if (e > best) { best = e; at = a; }
    }
    return at;
}
// the angle between two summed bearings (three 64-bit sums each, scale 2^32), fp64, rounded once
PF_HD float pf_trk_step(long long p0, long long p1, long long p2, long long c0, long long c1, long long c2) {
    if ((p0 == 0 && p1 == 0 && p2 == 0) || (c0 == 0 && c1 == 0 && c2 == 0)) return 0.f;
    const double inv = 1.0 / 4294967296.0;
    const double px = (double)p0 * inv, py = (double)p1 * inv, pz = (double)p2 * inv;
    const double cx = (double)c0 * inv, cy = (double)c1 * inv, cz = (double)c2 * inv;
    const double kx = py * cz - pz * cy, ky = pz * cx - px * cz, kz = px * cy - py * cx;
    const double n = sqrt((kx * kx + ky * ky) + kz * kz), d = (px * cx + py * cy) + pz * cz;
    return (float)atan2(n, d);
}
// the previous state of one image, read in full before anything is written (LDS on the device, copies in the emulation)
struct PfTrkPrev {
    const long long* area; const long long* bear;              // [M], [3 M] (slot-major: bear[3 a + k])
    const int* track; const int* age; const float* path;       // [M]
    int n_p, next_id;
};
// slot t of image b, as a current slot and as a previous one; rowbest, colbest [M]; fresh = the new slots below t, valid when
// slot t is new.  Writes the outputs and the state of slot t; every row beyond n_c (n_p) is zero.
PF_HD void pf_trk_slot(const PfTrkMatchArgs& g, const PfTrkPrev& p, long b, int t, int n_c, const int* rowbest, const int* colbest,
                       int fresh) {
    const long o = b * g.M + t;
    int track = 0, age = 0, origin = 0, fate = 0;
    float step = 0.f, path = 0.f;
    const long long* cs = g.sums + o * PF_SEG_SUMS;
    if (t < n_c) {
        const int a = colbest[t];
        if (a >= 0 && rowbest[a] == t) {
            track = p.track[a]; age = p.age[a] + 1; origin = track;
            step = pf_trk_step(p.bear[3 * a], p.bear[3 * a + 1], p.bear[3 * a + 2], cs[2], cs[3], cs[4]);
            path = p.path[a] + step;
        } else {
            track = p.next_id + fresh; age = 1; origin = a >= 0 ? p.track[a] : 0;
        }
    }
    if (t < p.n_p) {
        const int r = rowbest[t];
        if (r >= 0) fate = colbest[r] == t ? r + 1 : -(r + 1);
    }
    g.track[o] = track; g.age[o] = age; g.origin[o] = origin; g.fate[o] = fate; g.step[o] = step; g.path[o] = path;
    g.st_track[o] = track; g.st_age[o] = age; g.st_path[o] = path;
    for (int k = 0; k < PF_SEG_SUMS; ++k) g.st_sums[o * PF_SEG_SUMS + k] = cs[k];
}
PF_HD bool pf_trk_is_new(int t, int n_c, const int* rowbest, const int* colbest) {
    if (t >= n_c) return false;
    const int a = colbest[t];
    return !(a >= 0 && rowbest[a] == t);
}
PF_HD void pf_trk_paint_pixel(const PfTrkPaintArgs& a, long b, long n) {
    const long o = b * a.H * a.W + n;
    const int id = a.ids[o];
    a.track_map[o] = id > 0 && id <= a.M ? a.track[b * a.M + (id - 1)] : 0;
    a.st_ids[o] = id;
}

// ---- argument checks shared by the device entries and their host emulation ---------------------------------------------------
static inline int pf_trk_shape(int B, int H, int W, int M) {
    const int rc = pf_seg_geometry(B, H, W);
    if (rc != PF_OK) return rc;
    return M < 1 || M > PF_TRK_MAX_OBJECTS ? PF_ERR_BAD_SHAPE : PF_OK;
}
// every out[i] against every in[j] and every out[j], j < i
static inline bool pf_trk_overlap(const void* const* out, const long* outb, int n_out, const void* const* in, const long* inb, int n_in) {
    for (int i = 0; i < n_out; ++i) {
        for (int j = 0; j < n_in; ++j) if (pf_sg_meet(out[i], outb[i], in[j], inb[j])) return true;
        for (int j = 0; j < i; ++j) if (pf_sg_meet(out[i], outb[i], out[j], outb[j])) return true;
    }
    return false;
}
static inline int pf_trk_begin_check(void* votes, int B, int M) {
    if (!votes || pf_sg_misaligned(votes, 7)) return PF_ERR_BAD_ARG;
    return pf_trk_shape(B, 1, 1, M);
}
// fwd / bwd: filled in for the flows that are given; -> PF_OK
static inline int pf_trk_vote_check(const int* prev_ids, const int* ids, const float* flow_prev, const float* flow_cur,
                                    const unsigned char* mask_prev, const unsigned char* mask_cur, const float* rows, void* votes, int B,
                                    int H, int W, int M, PfTrkVoteArgs& fwd, PfTrkVoteArgs& bwd) {
    if (!prev_ids || !ids || !rows || !votes || (!flow_prev && !flow_cur)) return PF_ERR_BAD_ARG;
    if (pf_sg_misaligned(prev_ids, 3) || pf_sg_misaligned(ids, 3) || pf_sg_misaligned(flow_prev, 3) || pf_sg_misaligned(flow_cur, 3)
        || pf_sg_misaligned(rows, 3) || pf_sg_misaligned(votes, 7)) return PF_ERR_BAD_ARG;
    const int rc = pf_trk_shape(B, H, W, M);
    if (rc != PF_OK) return rc;
    const long N = (long)B * H * W;
    const void* out[1] = {votes};
    const long outb[1] = {(long)B * M * M * 8};
    const void* in[7] = {prev_ids, ids, flow_prev, flow_cur, mask_prev, mask_cur, rows};
    const long inb[7] = {N * 4, N * 4, N * 8, N * 8, N, N, (long)H * 8};
    if (pf_trk_overlap(out, outb, 1, in, inb, 7)) return PF_ERR_BAD_ARG;
    fwd.src = prev_ids; fwd.dst = ids; fwd.flow = flow_prev; fwd.mask = mask_prev; fwd.transposed = 0;
    bwd.src = ids; bwd.dst = prev_ids; bwd.flow = flow_cur; bwd.mask = mask_cur; bwd.transposed = 1;
    fwd.rows = bwd.rows = rows;
    fwd.S = bwd.S = static_cast<long long*>(votes);
    fwd.B = bwd.B = B; fwd.H = bwd.H = H; fwd.W = bwd.W = W; fwd.M = bwd.M = M;
    return PF_OK;
}
static inline int pf_trk_match_check(const void* votes, const int* count, const void* sums, int* st_count, void* st_sums, int* st_track,
                                     int* st_age, float* st_path, int* next_id, int* track, int* age, int* origin, int* fate,
                                     float* step, float* path, int B, int M, int n_dir, float min_overlap, PfTrkMatchArgs& a) {
    if (!votes || !count || !sums || !st_count || !st_sums || !st_track || !st_age || !st_path || !next_id || !track || !age || !origin
        || !fate || !step || !path) return PF_ERR_BAD_ARG;
    if (!(min_overlap > 0.f && min_overlap <= 1.f) || (n_dir != 1 && n_dir != 2)) return PF_ERR_BAD_ARG;       // a NaN compares false
    if (pf_sg_misaligned(votes, 7) || pf_sg_misaligned(sums, 7) || pf_sg_misaligned(st_sums, 7)) return PF_ERR_BAD_ARG;
    const void* all4[12] = {count, st_count, st_track, st_age, st_path, next_id, track, age, origin, fate, step, path};
    for (int i = 0; i < 12; ++i) if (pf_sg_misaligned(all4[i], 3)) return PF_ERR_BAD_ARG;
    const int rc = pf_trk_shape(B, 1, 1, M);
    if (rc != PF_OK) return rc;
    const long BM = (long)B * M;
    const void* in[3] = {votes, count, sums};
    const long inb[3] = {BM * M * 8, (long)B * 4, BM * 8 * PF_SEG_SUMS};
    const void* out[12] = {st_count, st_sums, st_track, st_age, st_path, next_id, track, age, origin, fate, step, path};
    const long outb[12] = {(long)B * 4, BM * 8 * PF_SEG_SUMS, BM * 4, BM * 4, BM * 4, (long)B * 4, BM * 4, BM * 4, BM * 4, BM * 4, BM * 4, BM * 4};
    if (pf_trk_overlap(out, outb, 12, in, inb, 3)) return PF_ERR_BAD_ARG;
    a.S = static_cast<const long long*>(votes); a.count = count; a.sums = static_cast<const long long*>(sums);
    a.st_count = st_count; a.st_sums = static_cast<long long*>(st_sums); a.st_track = st_track; a.st_age = st_age; a.st_path = st_path;
    a.next_id = next_id; a.track = track; a.age = age; a.origin = origin; a.fate = fate; a.step = step; a.path = path;
    a.B = B; a.M = M; a.n_dir = n_dir; a.min_overlap = min_overlap;
    return PF_OK;
}
static inline int pf_trk_paint_check(const int* ids, const int* track, int* track_map, int* st_ids, int B, int H, int W, int M,
                                     PfTrkPaintArgs& a) {
    if (!ids || !track || !track_map || !st_ids) return PF_ERR_BAD_ARG;
    if (pf_sg_misaligned(ids, 3) || pf_sg_misaligned(track, 3) || pf_sg_misaligned(track_map, 3) || pf_sg_misaligned(st_ids, 3))
        return PF_ERR_BAD_ARG;
    const int rc = pf_trk_shape(B, H, W, M);
    if (rc != PF_OK) return rc;
    const long N = (long)B * H * W;
    const void* in[2] = {ids, track};
    const long inb[2] = {N * 4, (long)B * M * 4};
    const void* out[2] = {track_map, st_ids};
    const long outb[2] = {N * 4, N * 4};
    if (pf_trk_overlap(out, outb, 2, in, inb, 2)) return PF_ERR_BAD_ARG;
    a.ids = ids; a.track = track; a.track_map = track_map; a.st_ids = st_ids; a.B = B; a.H = H; a.W = W; a.M = M;
    return PF_OK;
}
