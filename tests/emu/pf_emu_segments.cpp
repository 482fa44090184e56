// Host emulation of pf_seg_tables / pf_seg_label / pf_seg_objects -- TEST INFRASTRUCTURE ONLY (its own library,
// libpf_emu_segments.so).  The union function, the merge items, the per-pixel sums, the object table and the argument checks are
// prior-flow_amd/csrc/pf_segments.h, the file the device kernels compile; a launch is restated as a loop over its grid, an atomic
// minimum or add as a plain one.  The product never loads this library.
//
// pf_emu_seg_order picks the order in which the merge loop visits its items (and the pole rows their pixels): 0 in order, 1
// reversed, any other value a fixed pseudo-random permutation seeded with it.  The labels must not notice
// (tests/test_segments_host.py).
#include <algorithm>
#include <numeric>
#include <vector>

#include "pf_segments.h"

static unsigned long long g_order = 0;
extern "C" void pf_emu_seg_order(unsigned long long seed) { g_order = seed; }

static std::vector<long> visit_order(long N) {
    std::vector<long> order(N);
    std::iota(order.begin(), order.end(), 0L);
    if (g_order == 1) std::reverse(order.begin(), order.end());
    else if (g_order > 1) {
        unsigned long long s = g_order;
        for (long i = N - 1; i > 0; --i) {                     // Fisher-Yates on a 64-bit LCG
            s = s * 6364136223846793005ULL + 1442695040888963407ULL;
            std::swap(order[i], order[(long)((s >> 33) % (unsigned long long)(i + 1))]);
        }
    }
    return order;
}

extern "C" long pf_seg_scratch_bytes(int B, int H, int W) { return pf_seg_bytes(B, H, W); }

extern "C" int pf_seg_tables(float* rows, float* cols, int H, int W, void*) {
    const int rc = pf_seg_tables_check(rows, cols, H, W);
    if (rc != PF_OK) return rc;
    for (int y = 0; y < H; ++y) pf_seg_row(y, H, rows[2 * y], rows[2 * y + 1]);
    for (int x = 0; x < W; ++x) pf_seg_col(x, W, cols[2 * x], cols[2 * x + 1]);
    return PF_OK;
}

// one tile: the runs of every row, every vertical and diagonal link inside the tile, then the tile's roots as global indices
static void label_tile(const PfSegLabelArgs& a, long base, int y0, int x0) {
    int lab[PF_SG_TH * PF_SG_TW];
    const int H = a.H, W = a.W;
    auto set = [&](int r, int c) {
        return r >= 0 && c >= 0 && c < PF_SG_TW && y0 + r < H && x0 + c < W && pf_seg_set(a.mask[base + (long)(y0 + r) * W + x0 + c]);
    };
    for (int r = 0; r < PF_SG_TH; ++r) {
        int start = 0;
        for (int c = 0; c < PF_SG_TW; ++c) {
            if (!set(r, c)) { lab[r * PF_SG_TW + c] = -1; start = c + 1; }
            else lab[r * PF_SG_TW + c] = r * PF_SG_TW + start;
        }
    }
    const PfSegPlain m{lab};
    for (int r = 1; r < PF_SG_TH; ++r)
        for (int c = 0; c < PF_SG_TW; ++c) {
            if (!set(r, c)) continue;
            const int i = r * PF_SG_TW + c, u = (r - 1) * PF_SG_TW + c;
            if (set(r - 1, c)) pf_seg_unite(m, i, u);
            if (a.conn == 8) {
                if (set(r - 1, c - 1)) pf_seg_unite(m, i, u - 1);
                if (set(r - 1, c + 1)) pf_seg_unite(m, i, u + 1);
            }
        }
    for (int r = 0; r < PF_SG_TH && y0 + r < H; ++r)
        for (int c = 0; c < PF_SG_TW && x0 + c < W; ++c) {
            const int v = lab[r * PF_SG_TW + c];
            int g = -1;
            if (v >= 0) {
                const int root = pf_seg_find(m, v);
                g = (y0 + root / PF_SG_TW) * W + x0 + root % PF_SG_TW;
            }
            a.parent[base + (long)(y0 + r) * W + x0 + c] = g;
            a.area[base + (long)(y0 + r) * W + x0 + c] = 0;
        }
}

extern "C" int pf_seg_label(const unsigned char* mask, const float* rows, int* labels, void* scratch, long scratch_bytes, int B, int H,
                            int W, int connectivity, int poles, void*) {
    PfSegLabelArgs a;
    const int rc = pf_seg_label_check(mask, rows, labels, scratch, scratch_bytes, B, H, W, connectivity, poles, a);
    if (rc != PF_OK) return rc;
    const long N = (long)H * W;
    for (long b = 0; b < B; ++b) {
        for (int y0 = 0; y0 < H; y0 += PF_SG_TH)
            for (int x0 = 0; x0 < W; x0 += PF_SG_TW) label_tile(a, b * N, y0, x0);
        const PfSegPlain m{a.parent + b * N};
        for (long t : visit_order(pf_seg_merge_items(H, W))) pf_seg_merge_item(m, t, H, W, connectivity);
        for (int pole = 0; pole < (poles ? 2 : 0); ++pole) {
            const int off = (pole == 0 ? 0 : H - 1) * W;
            int an = W;
            for (int x = 0; x < W && an == W; ++x) if (m.load(off + x) >= 0) an = x;
            if (an == W) continue;
            for (long x : visit_order(W)) if (x != an && m.load(off + (int)x) >= 0) pf_seg_unite(m, off + (int)x, off + an);
        }
        for (long n : visit_order(N)) {
            int root = -1;
            if (m.load((int)n) >= 0) {
                root = pf_seg_find(m, (int)n);
                a.area[b * N + root] += pf_seg_area_q(rows[2 * (int)(n / W)]);
            }
            labels[b * N + n] = root + 1;
        }
    }
    return PF_OK;
}

extern "C" int pf_seg_objects(const int* labels, const float* values, const float* rows, const float* cols, void* scratch,
                              long scratch_bytes, int* ids, unsigned char* keep, int* roots, int* count, float* table, void* sums, int B,
                              int C, int H, int W, int max_objects, float min_area, void*) {
    PfSegObjArgs a;
    const int rc = pf_seg_objects_check(labels, values, rows, cols, scratch, scratch_bytes, ids, keep, roots, count, table, sums, B, C, H,
                                        W, max_objects, min_area, a);
    if (rc != PF_OK) return rc;
    const long N = (long)H * W;
    const int M = max_objects;
    for (long b = 0; b < B; ++b) {
        for (int y = 0; y < H; ++y) {                                   // count
            int c = 0;
            for (int x = 0; x < W; ++x) c += pf_seg_survivor(a, b * N + (long)y * W + x, y * W + x) ? 1 : 0;
            a.rowcount[b * H + y] = c;
        }
        int run = 0;                                                    // scan
        for (int y = 0; y < H; ++y) { a.rowbase[b * H + y] = run; run += a.rowcount[b * H + y]; }
        count[b] = run;
        for (int k = 0; k < M; ++k) roots[b * M + k] = -1;
        for (int k = 0; k < M * PF_SEG_SUMS; ++k) a.sums[b * M * PF_SEG_SUMS + k] = 0;
        for (int y = 0; y < H; ++y) {                                   // assign
            int r = a.rowbase[b * H + y];
            for (int x = 0; x < W; ++x) {
                const long o = b * N + (long)y * W + x;
                const bool sv = pf_seg_survivor(a, o, y * W + x);
                a.rank[o] = sv ? ++r : 0;
                if (sv && r <= M) roots[b * M + (r - 1)] = y * W + x;
            }
        }
        const int used = C > 0 ? 6 + C : 5;
        for (long n : visit_order(N)) {                                 // accumulate
            int id;
            pf_seg_pixel_ids(a, b, n, id);
            if (id <= 0) continue;
            long long s[PF_SEG_SUMS];
            pf_seg_pixel_sums(a, b, (int)(n / W), (int)(n % W), s);
            for (int k = 0; k < used; ++k) a.sums[(b * M + (id - 1)) * PF_SEG_SUMS + k] += s[k];
        }
        for (int k = 0; k < M; ++k) pf_seg_resolve_object(a, b, k);     // resolve
    }
    return PF_OK;
}

extern "C" const char* pf_version(void) { return "priorflow segments host emulation (tests only)"; }
