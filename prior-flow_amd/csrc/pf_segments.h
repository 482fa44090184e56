// Moving objects: connected components of a byte mask on the cyclic panorama, per-component sums and a dense, capped object table
// (include/priorflow_hip.h: pf_seg_tables, pf_seg_label, pf_seg_objects).  The statement, once, for the
// device kernels (pf_segments.hip), the host emulation (tests/emu/pf_emu_segments.cpp) and the C checks.  The row and column
// angles, pf_vp_dir and pf_vp_erp are pf_viewport.h's, the quantiser pf_egomotion.h's; nothing of them is restated here.
//
// Labels.  A pixel is SET when its mask byte is non-zero.  Neighbours: connectivity 4 or 8; x is cyclic, so (W-1, y) and (0, y)
// are horizontal neighbours and, at 8, (W-1, y) and (0, y+-1) diagonal ones; rows do not wrap; with poles = 1 all set pixels of
// row 0 are one component and so are those of row H-1.  label = 1 + min(y W + x) over the component, background 0: a function of
// the mask alone.
//
// Union-find.  parent[i] = -1 for background, else the linear index of a pixel of i's component with parent[i] <= i; a root holds
// itself.  pf_seg_unite(a, b): find both roots; while they differ, atomic-min the SMALLER root into the LARGER root's cell; if the
// cell still held the larger root, the link is made; otherwise another thread had already lowered it to `old` < larger root, and
// the pair (old, smaller root) is united instead.  Termination: every cell only ever decreases and stays >= 0 (an atomic min of
// an index of its own component that is smaller than the cell's index), every find walks strictly downwards, and each turn of
// the loop either ends it or replaces the pair's larger root by a strictly smaller index; the indices are bounded below by 0.
// Correctness: a cell is only ever lowered to an index of the same component, so trees never mix components; when the loop ends
// the two pixels have one root.  The final root of a component is its smallest index whatever the order of the unions, because
// the smallest index can never get a parent below itself.
//
// Tables, once per geometry: rows [H,2] = (cos phi, sin phi) of pf_vp_phi(y), cols [W,2] = (cos theta, sin theta) of pf_vp_theta(x).
// Every later step reads them; no transcendental is evaluated per pixel.
//
// Sums per object, PF_SEG_SUMS = 10 64-bit integers, a contribution pf_ego_quant(value, scale) of ONE fp32 value:
//   0 area    cos phi                     scale 2^32        1 pixels   1
//   2..4      cos phi * p, p = pf_vp_dir(cols[x], rows[y]): each a product of two fp32 numbers, rounded once (products only:
//             nothing for a compiler to contract)           scale 2^32
//   5 value weight   cos phi over the pixels ALL of whose C channels satisfy |v| < PF_SEG_VMAX = 2^16 (a NaN compares false)
//   6..9      cos phi * v_c over the same pixels            scale 2^16
// Bound: cos phi <= 1, |p| <= 1, |v| < 2^16 and H W < 2^30, so every sum stays below 2^30 2^32 = 2^62 in magnitude.
//
// Objects.  A component survives when its area sum is at least ceil(min_area 2^32).  Survivors are numbered 1, 2, ... by their
// root's linear index; ids beyond max_objects = M are 0; count [B] is the number of survivors, not clipped.  keep marks the set
// pixels of every survivor.  roots [B,M] holds the root index, -1 where unused.  table [B,M,6+C], resolved in fp64 from the sums:
// area, pixels, centroid x, y (pf_vp_erp of the summed bearing; (0, 0) when the three sums are zero), |sum w p| / sum w, value
// weight, C means (0 when the weight is zero).  Unused rows are zero.  No address depends on an input value other than through
// labels the kernels wrote themselves.
#pragma once
#include <string.h>

#include "pf_egomotion.h"

#define PF_SG_VMAX 65536.f
#define PF_SG_F 4294967296.f                 // 2^32
#define PF_SG_FV 65536.f                     // 2^16
#define PF_SG_TW 64                          // a tile is PF_SG_TW columns wide: one wave holds a row of it
#ifndef PF_SG_TH                             // rows of a tile; profiles/time_segments.py --lib times builds with 16 and 64
#define PF_SG_TH 32
#endif
static_assert(PF_SEG_SUMS == 10 && PF_SEG_MAX_OBJECTS == 4096 && PF_SEG_COLS == 6, "the sizes of pf_segments.h and of the public header");

struct PfSegLabelArgs {
    const unsigned char* mask; const float* rows; int* labels; int* parent; long long* area;   // [B,H,W] maps, rows [H,2]
    int B, H, W, conn, poles;
};
struct PfSegObjArgs {
    const int* labels; const float* values; const float* rows; const float* cols;              // values [B,C,H,W] or null
    const long long* area; int* rank; int* rowcount; int* rowbase;                              // scratch
    int* ids; unsigned char* keep; int* roots; int* count; float* table; long long* sums;       // outputs
    int B, C, H, W, M; long long min_q;
};

PF_HD bool pf_seg_set(unsigned char m) { return m != 0; }
// (cos phi, sin phi) of row y and (cos theta, sin theta) of column x; cos phi is never negative
PF_HD void pf_seg_row(int y, int H, float& c, float& s) { pf_ego_row(y, H, c, s); c = c < 0.f ? 0.f : c; }
PF_HD void pf_seg_col(int x, int W, float& c, float& s) { const float t = pf_vp_theta((float)x, W); c = cosf(t); s = sinf(t); }

// ---- union-find over any memory: M has load(i) and min(i, v) -> the value before -------------------------------------------------
template <class M>
PF_HD int pf_seg_find(const M& m, int i) {
    int p = m.load(i);
    while (p != i) { i = p; p = m.load(i); }                     // strictly downwards: parent <= index
    return i;
}
template <class M>
PF_HD void pf_seg_unite(const M& m, int a, int b) {
    a = pf_seg_find(m, a); b = pf_seg_find(m, b);
    while (a != b) {
        if (a < b) { const int t = a; a = b; b = t; }            // a: the larger root
        const int old = m.min(a, b);
        if (old == a) return;                                    // a was still a root: linked
        a = pf_seg_find(m, old); b = pf_seg_find(m, b);          // old < a: each turn strictly lowers the larger index
    }
}
// plain memory (the host emulation, and device code on memory no other thread writes)
struct PfSegPlain {
    int* p;
    PF_HD int load(int i) const { return p[i]; }
    PF_HD int min(int i, int v) const { const int o = p[i]; if (v < o) p[i] = v; return o; }
};

// ---- merge: what one border pixel unites --------------------------------------------------------------------------------------
// the borders of image b: rows k PF_SG_TH (k >= 1) and columns k PF_SG_TW (k >= 0; column 0 is the seam)
PF_HD long pf_seg_merge_items(int H, int W) {
    const long hb = (H - 1) / PF_SG_TH, vb = (W + PF_SG_TW - 1) / PF_SG_TW;
    return hb * W + vb * H;
}
// item t of pf_seg_merge_items; m: image b's parent plane
template <class M>
PF_HD void pf_seg_merge_item(const M& m, long t, int H, int W, int conn) {
    const long hb = (H - 1) / PF_SG_TH;
    if (t < hb * W) {                                            // a pixel below a horizontal border against the row above
        const int y = ((int)(t / W) + 1) * PF_SG_TH, x = (int)(t % W), i = y * W + x;
        if (m.load(i) < 0) return;
        const int up = (y - 1) * W;
        if (m.load(up + x) >= 0) pf_seg_unite(m, i, up + x);
        if (conn == 8) {
            const int xl = x == 0 ? W - 1 : x - 1, xr = x + 1 == W ? 0 : x + 1;
            if (m.load(up + xl) >= 0) pf_seg_unite(m, i, up + xl);
            if (m.load(up + xr) >= 0) pf_seg_unite(m, i, up + xr);
        }
    } else {                                                     // a pixel right of a vertical border against the column before it
        t -= hb * W;
        const int x = (int)(t / H) * PF_SG_TW, y = (int)(t % H), i = y * W + x;
        if (m.load(i) < 0) return;
        const int xl = x == 0 ? W - 1 : x - 1;
        if (m.load(y * W + xl) >= 0) pf_seg_unite(m, i, y * W + xl);
        if (conn == 8) {
            if (y > 0 && m.load((y - 1) * W + xl) >= 0) pf_seg_unite(m, i, (y - 1) * W + xl);
            if (y + 1 < H && m.load((y + 1) * W + xl) >= 0) pf_seg_unite(m, i, (y + 1) * W + xl);
        }
    }
}

// ---- sums ----------------------------------------------------------------------------------------------------------------------
PF_HD long long pf_seg_area_q(float cp) { return pf_ego_quant(cp, PF_SG_F); }
PF_HD bool pf_seg_value_ok(float v) { return fabsf(v) < PF_SG_VMAX; }                      // a NaN compares false
// the contributions s[PF_SEG_SUMS] of pixel (x, y) of image b
PF_HD void pf_seg_pixel_sums(const PfSegObjArgs& a, long b, int y, int x, long long* s) {
    const float cp = a.rows[2 * y], sp = a.rows[2 * y + 1], ct = a.cols[2 * x], st = a.cols[2 * x + 1];
    const PfVec3 p = pf_vp_dir(ct, st, cp, sp);
    const float wx = cp * p.x, wy = cp * p.y, wz = cp * p.z;
    s[0] = pf_seg_area_q(cp); s[1] = 1;
    s[2] = pf_ego_quant(wx, PF_SG_F); s[3] = pf_ego_quant(wy, PF_SG_F); s[4] = pf_ego_quant(wz, PF_SG_F);
    s[5] = 0; s[6] = 0; s[7] = 0; s[8] = 0; s[9] = 0;
    if (a.C > 0) {
        const long N = (long)a.H * a.W;
        const float* v = a.values + b * a.C * N + ((long)y * a.W + x);
        const float v0 = v[0], v1 = a.C > 1 ? v[N] : 0.f, v2 = a.C > 2 ? v[2 * N] : 0.f, v3 = a.C > 3 ? v[3 * N] : 0.f;
        if (pf_seg_value_ok(v0) && pf_seg_value_ok(v1) && pf_seg_value_ok(v2) && pf_seg_value_ok(v3)) {
            const float q0 = cp * v0, q1 = cp * v1, q2 = cp * v2, q3 = cp * v3;
            s[5] = s[0];
            s[6] = pf_ego_quant(q0, PF_SG_FV); s[7] = pf_ego_quant(q1, PF_SG_FV); s[8] = pf_ego_quant(q2, PF_SG_FV);
            s[9] = pf_ego_quant(q3, PF_SG_FV);
        }
    }
}
// a root cell's rank decision: does the component of root i (its own label, its area sum) survive
PF_HD bool pf_seg_survivor(const PfSegObjArgs& a, long o, int i) { return a.labels[o] == i + 1 && a.area[o] >= a.min_q; }
// what pixel n of image b gets: rank = the 1-based number of its component among the survivors, 0 when it did not survive
PF_HD void pf_seg_pixel_ids(const PfSegObjArgs& a, long b, long n, int& id) {
    const long N = (long)a.H * a.W, o = b * N + n;
    const int l = a.labels[o];
    const int r = l > 0 ? a.rank[b * N + (l - 1)] : 0;
    a.keep[o] = r > 0 ? 1 : 0;
    id = r <= a.M ? r : 0;
    a.ids[o] = id;
}
// object k (0-based) of image b
PF_HD void pf_seg_resolve_object(const PfSegObjArgs& a, long b, int k) {
    const long long* s = a.sums + (b * a.M + k) * PF_SEG_SUMS;
    float* t = a.table + (b * a.M + k) * (PF_SEG_COLS + a.C);
    const double inv = 1.0 / 4294967296.0, invv = 1.0 / 65536.0;
    const double area = (double)s[0] * inv;
    float cx = 0.f, cy = 0.f, res = 0.f;
    if (s[2] != 0 || s[3] != 0 || s[4] != 0) {
        const double bx = (double)s[2] * inv, by = (double)s[3] * inv, bz = (double)s[4] * inv;
        const double nrm = sqrt((bx * bx + by * by) + bz * bz);
        PfVec3 d;
        d.x = (float)(bx / nrm); d.y = (float)(by / nrm); d.z = (float)(bz / nrm);
        pf_vp_erp(d, a.H, a.W, cx, cy);
        if (s[0] > 0) res = (float)(nrm / area);
    }
    t[0] = (float)area; t[1] = (float)s[1]; t[2] = cx; t[3] = cy; t[4] = res;
    const double vw = (double)s[5] * inv;
    t[5] = (float)vw;
    for (int c = 0; c < a.C; ++c) t[PF_SEG_COLS + c] = s[5] > 0 ? (float)(((double)s[6 + c] * invv) / vw) : 0.f;
}

// ---- argument checks shared by the device entries and their host emulation ---------------------------------------------------
static inline bool pf_sg_meet(const void* p, long np, const void* q, long nq) {
    if (!p || !q) return false;
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + (uintptr_t)nq && b < a + (uintptr_t)np;
}
static inline bool pf_sg_misaligned(const void* p, int mask) { return ((uintptr_t)p & (uintptr_t)mask) != 0; }
static inline int pf_seg_geometry(int B, int H, int W) {
    if (B < 1 || H < 1 || W < 1 || (long)H * W >= (1L << 30) || B > PF_EGO_MAX_GRID) return PF_ERR_BAD_SHAPE;
    return PF_OK;
}
// scratch: area int64 [B,H,W], parent, rank int32 [B,H,W], rowcount, rowbase int32 [B,H]
static inline long pf_seg_bytes(int B, int H, int W) {
    const int rc = pf_seg_geometry(B, H, W);
    return rc != PF_OK ? rc : (long)B * H * W * 16 + (long)B * H * 8;
}
struct PfSegScratch { long long* area; int* parent; int* rank; int* rowcount; int* rowbase; };
static inline PfSegScratch pf_seg_carve(void* scratch, int B, int H, int W) {
    const long N = (long)B * H * W;
    PfSegScratch s;
    s.area = static_cast<long long*>(scratch);
    s.parent = reinterpret_cast<int*>(s.area + N);
    s.rank = s.parent + N;
    s.rowcount = s.rank + N;
    s.rowbase = s.rowcount + (long)B * H;
    return s;
}
static inline int pf_seg_tables_check(float* rows, float* cols, int H, int W) {
    if (!rows || !cols || pf_sg_misaligned(rows, 3) || pf_sg_misaligned(cols, 3)) return PF_ERR_BAD_ARG;
    const int rc = pf_seg_geometry(1, H, W);
    if (rc != PF_OK) return rc;
    if (pf_sg_meet(rows, (long)H * 8, cols, (long)W * 8)) return PF_ERR_BAD_ARG;
    return PF_OK;
}
static inline int pf_seg_label_check(const unsigned char* mask, const float* rows, int* labels, void* scratch, long scratch_bytes, int B,
                                     int H, int W, int connectivity, int poles, PfSegLabelArgs& a) {
    if (!mask || !rows || !labels || !scratch) return PF_ERR_BAD_ARG;
    if (pf_sg_misaligned(rows, 3) || pf_sg_misaligned(labels, 3) || pf_sg_misaligned(scratch, 7)) return PF_ERR_BAD_ARG;
    if ((connectivity != 4 && connectivity != 8) || (poles != 0 && poles != 1)) return PF_ERR_BAD_ARG;
    const int rc = pf_seg_geometry(B, H, W);
    if (rc != PF_OK) return rc;
    const long need = pf_seg_bytes(B, H, W), N = (long)B * H * W;
    if (scratch_bytes < need) return PF_ERR_BAD_ARG;
    if (pf_sg_meet(labels, N * 4, mask, N) || pf_sg_meet(labels, N * 4, rows, (long)H * 8) || pf_sg_meet(scratch, need, mask, N)
        || pf_sg_meet(scratch, need, rows, (long)H * 8) || pf_sg_meet(scratch, need, labels, N * 4)) return PF_ERR_BAD_ARG;
    const PfSegScratch s = pf_seg_carve(scratch, B, H, W);
    a.mask = mask; a.rows = rows; a.labels = labels; a.parent = s.parent; a.area = s.area;
    a.B = B; a.H = H; a.W = W; a.conn = connectivity; a.poles = poles;
    return PF_OK;
}
static inline int pf_seg_objects_check(const int* labels, const float* values, const float* rows, const float* cols, void* scratch,
                                       long scratch_bytes, int* ids, unsigned char* keep, int* roots, int* count, float* table,
                                       void* sums, int B, int C, int H, int W, int max_objects, float min_area, PfSegObjArgs& a) {
    if (!labels || !rows || !cols || !scratch || !ids || !keep || !roots || !count || !table || !sums) return PF_ERR_BAD_ARG;
    if (C < 0 || C > 4 || (C > 0) != (values != nullptr)) return PF_ERR_BAD_ARG;
    if (max_objects < 1 || max_objects > PF_SEG_MAX_OBJECTS) return PF_ERR_BAD_ARG;
    if (!(min_area >= 0.f && min_area <= PF_EGO_FAR)) return PF_ERR_BAD_ARG;                  // a NaN compares false
    if (pf_sg_misaligned(labels, 3) || pf_sg_misaligned(values, 3) || pf_sg_misaligned(rows, 3) || pf_sg_misaligned(cols, 3)
        || pf_sg_misaligned(scratch, 7) || pf_sg_misaligned(ids, 3) || pf_sg_misaligned(roots, 3) || pf_sg_misaligned(count, 3)
        || pf_sg_misaligned(table, 3) || pf_sg_misaligned(sums, 7)) return PF_ERR_BAD_ARG;
    const int rc = pf_seg_geometry(B, H, W);
    if (rc != PF_OK) return rc;
    const long need = pf_seg_bytes(B, H, W), N = (long)B * H * W, BM = (long)B * max_objects;
    if (scratch_bytes < need) return PF_ERR_BAD_ARG;
    const void* in[5] = {labels, values, rows, cols, scratch};
    const long inb[5] = {N * 4, N * 4 * C, (long)H * 8, (long)W * 8, need};
    const void* out[6] = {ids, keep, roots, count, table, sums};
    const long outb[6] = {N * 4, N, BM * 4, (long)B * 4, BM * 4 * (PF_SEG_COLS + C), BM * 8 * PF_SEG_SUMS};
    for (int i = 0; i < 6; ++i) {
        for (int j = 0; j < 5; ++j) if (pf_sg_meet(out[i], outb[i], in[j], inb[j])) return PF_ERR_BAD_ARG;
        for (int j = 0; j < i; ++j) if (pf_sg_meet(out[i], outb[i], out[j], outb[j])) return PF_ERR_BAD_ARG;
    }
    const PfSegScratch s = pf_seg_carve(scratch, B, H, W);
    a.labels = labels; a.values = values; a.rows = rows; a.cols = cols; a.area = s.area; a.rank = s.rank; a.rowcount = s.rowcount;
    a.rowbase = s.rowbase; a.ids = ids; a.keep = keep; a.roots = roots; a.count = count; a.table = table;
    a.sums = static_cast<long long*>(sums); a.B = B; a.C = C; a.H = H; a.W = W; a.M = max_objects;
    a.min_q = (long long)ceil((double)min_area * 4294967296.0);
    return PF_OK;
}
