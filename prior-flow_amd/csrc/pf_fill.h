// Push-pull hole filling on the cyclic panorama (include/priorflow_hip.h: pf_fill_*).  The statement, once,
// for the device kernels (pf_fill.hip), the host emulation (tests/emu/pf_emu_fill.cpp) and the C checks.  Every step is one
// rounded fp32 operation in the order written here (the units are built without contraction).
//
// Inputs: src fp32 [B,C,H,W] (C = 1..4), hole uint8 [B,H,W] (non-zero: missing), optionally weight fp32 [B,H,W].
// Level-0 weight: w0 = 0 when the hole byte is set, when one of the C values is not finite or |v| >= 2^30 (PF_FILL_FAR), or when a
//   given weight is not finite or <= 0; otherwise min(weight, 1), or 1 without a weight map.  A value at a pixel with w = 0 never
//   enters arithmetic (select, not multiply): a NaN under a hole cannot leak.
// Levels: H_(l+1) = max(1, ceil(H_l / 2)), the same for W, until the level is 1 x 1; L = pf_fill_levels(H, W) pulls.
// Pull: coarse cell (j, i) takes the fine cells (2j + dy, 2i + dx), dy outer, dx inner, that lie inside the fine level and have
//   w > 0:  s = 0, n_c = 0;  per taken cell s = s + w, n_c = n_c + w * v_c;  V_c = n_c / s when s > 0, else 0;  S = min(1, s).
//   No wrap: an odd last column or row stands alone.
// Apex: the 1 x 1 level counts as known with its value (0 when its weight is 0); empty[b] = 1 exactly when that weight is 0.
// Push, from the filled coarse level U to the fine level (v, w): a fine cell with w >= 1 keeps v, the same bits.  Otherwise the
//   x taps are (x/2 - 1, x/2) with t = 0.75 for an even x and ((x-1)/2, (x+1)/2) with t = 0.25 for an odd one, the same in y;
//   columns are wrapped into [0, W_(l+1)), rows clamped into [0, H_(l+1) - 1];  lerp(a, b, t) = a + t * (b - a);
//   u = lerp(lerp(U00, U01, tx), lerp(U10, U11, tx), ty) (first index: the y tap);  the cell becomes u when w <= 0, else
//   lerp(u, v, w).  Level 0's result is out.
// Division: the fp32 `/` of both builds is the correctly rounded one (hipcc's default for HIP, IEEE on the host), and neither
//   build flushes fp32 denormals, so no fp64 detour is needed; tests/test_hip_fill.py holds the device to the host bit for bit.
//
// The statement is per level and per element, so every fusion of levels gives the bits of the level-by-level form.  The fused
// form (pf_fill_pushpull) is written here as per-thread phases between barriers; the device kernels put __syncthreads() between
// them, the emulation loops over the threads of a workgroup.
//
// Scratch, in floats (pf_fill_bytes / 4): w0 [B,H,W], then for l = 1..L the values [B,C,H_l,W_l] and the weights [B,H_l,W_l] of
// level l (pf_fill_level_off).  Every cell is written before it is read: scratch may hold anything on entry.
#pragma once
#include "pf_common.h"
#include "../../include/priorflow_hip.h"      // checks the definitions against their declarations

#define PF_FILL_FAR 1073741824.f              // 2^30
#define PF_FILL_MAX_GRID 65535
#define PF_FILL_MAX_LEVELS 30                 // H * W < 2^30
#define PF_FILL_TH 32                         // the fused kernels' level-0 tile
#define PF_FILL_TW 64
#define PF_FILL_THREADS 256
#define PF_FILL_TILE_LEVELS 5                 // levels a tile kernel reduces / expands through LDS
#define PF_FILL_APEX_THREADS 1024
#define PF_FILL_APEX_FLOATS 1024              // LDS of the apex kernel for the levels above the one it streams
#define PF_FILL_PT_CELLS (16 * 32 + 8 * 16 + 4 * 8 + 2 * 4 + 1 * 2)
#define PF_FILL_PT_FLOATS (5 * PF_FILL_PT_CELLS)        // pull tile: levels 1..5 of a tile, C + 1 <= 5 planes
#define PF_FILL_R1 (20 * 36)                  // push tile: the region of level l is at most (32 >> l) + 4 by (64 >> l) + 4 cells
#define PF_FILL_R2 (12 * 20)
#define PF_FILL_R3 (8 * 12)
#define PF_FILL_R4 (6 * 8)
#define PF_FILL_R5 (5 * 6)
#define PF_FILL_PU_FLOATS (4 * (PF_FILL_R1 + PF_FILL_R2 + PF_FILL_R3 + PF_FILL_R4 + PF_FILL_R5))

struct PfFill4 { float v0, v1, v2, v3; };
struct PfFillArgs {
    const float* src; const unsigned char* hole; const float* weight; float* out; unsigned char* empty; float* scratch;
    int B, C, H, W, L, P, S;                  // L pulls; the tile kernels cover levels 0..P; the apex kernel streams level S
};

// ---- geometry -----------------------------------------------------------------------------------------------------------------
PF_HD int pf_fill_half(int n) { return n > 1 ? (n + 1) / 2 : 1; }
PF_HD void pf_fill_dims(int H, int W, int l, int& h, int& w) {
    h = H; w = W;
    for (int k = 0; k < l; ++k) { h = pf_fill_half(h); w = pf_fill_half(w); }
}
PF_HD int pf_fill_count_levels(int H, int W) {
    int l = 0;
    while (H > 1 || W > 1) { H = pf_fill_half(H); W = pf_fill_half(W); ++l; }
    return l;
}
// where level l >= 1 starts in scratch (its values; its weights follow B * C * H_l * W_l floats later); l = L + 1: the total
PF_HD long pf_fill_level_off(int B, int C, int H, int W, int l) {
    long o = (long)B * H * W;
    int h = H, w = W;
    for (int k = 1; k < l; ++k) {
        h = pf_fill_half(h); w = pf_fill_half(w);
        o += (long)B * (C + 1) * h * w;
    }
    return o;
}
// floats of the levels l + 1 .. L of ONE image, C + 1 planes each: what the apex kernel keeps in LDS when it streams level l
PF_HD long pf_fill_above(int C, int H, int W, int l, int L) {
    int h, w;
    pf_fill_dims(H, W, l, h, w);
    long n = 0;
    for (int k = l; k < L; ++k) {
        h = pf_fill_half(h); w = pf_fill_half(w);
        n += (long)(C + 1) * h * w;
    }
    return n;
}
// the split of the levels between the fused kernels, from the shape alone (pf_fill_bytes and pf_fill_pushpull both use it): the
// tile kernels take levels 0..P, the apex kernel streams level S (the first at or above P whose upper levels fit its LDS) and
// holds S + 1 .. L; the levels between P and S, on maps too large for that, go level by level.
static inline void pf_fill_plan(int C, int H, int W, int& L, int& P, int& S) {
    L = pf_fill_count_levels(H, W);
    P = L < PF_FILL_TILE_LEVELS ? L : PF_FILL_TILE_LEVELS;
    S = P;
    while (pf_fill_above(C, H, W, S, L) > PF_FILL_APEX_FLOATS) ++S;
}

// ---- the arithmetic ---------------------------------------------------------------------------------------------------------------
PF_HD float pf_fill_lerp(float a, float b, float t) { const float d = b - a; const float p = t * d; return a + p; }
PF_HD bool pf_fill_usable(float v) { return fabsf(v) < PF_FILL_FAR; }                // a NaN compares false
// src, hole, weight: at image b; n: the pixel
// (every load is made whatever the others give, so that they are in flight together; the choice comes afterwards)
PF_HD float pf_fill_w0(const float* src, const unsigned char* hole, const float* weight, int C, long N, long n) {
    const unsigned char h = hole[n];
    const float v0 = src[n], v1 = C > 1 ? src[N + n] : 0.f, v2 = C > 2 ? src[2 * N + n] : 0.f, v3 = C > 3 ? src[3 * N + n] : 0.f;
    const float w = weight ? weight[n] : 1.f;
    const bool ok = (h == 0) & pf_fill_usable(v0) & pf_fill_usable(v1) & pf_fill_usable(v2) & pf_fill_usable(v3)
                    & (w > 0.f) & (w <= 3.402823466e38f);
    return ok ? (w < 1.f ? w : 1.f) : 0.f;
}
// a level as maps in memory (global, or LDS through a generic pointer): values [C][h][width], weights [h][width]
struct PfFillMap {
    const float* v; const float* w; int width; long plane;
    PF_HD float wt(int y, int x) const { return w[(long)y * width + x]; }
    PF_HD float val(int c, int y, int x) const { return v[c * plane + (long)y * width + x]; }
};
// level 0 with its weight computed on the fly
struct PfFillSrc {
    const float* src; const unsigned char* hole; const float* weight; int C, width; long plane;
    PF_HD float wt(int y, int x) const { return pf_fill_w0(src, hole, weight, C, plane, (long)y * width + x); }
    PF_HD float val(int c, int y, int x) const { return src[c * plane + (long)y * width + x]; }
};
PF_HD PfFillSrc pf_fill_src(const PfFillArgs& a, long b) {
    PfFillSrc s;
    s.plane = (long)a.H * a.W; s.width = a.W; s.C = a.C;
    s.src = a.src + b * a.C * s.plane; s.hole = a.hole + b * s.plane; s.weight = a.weight ? a.weight + b * s.plane : nullptr;
    return s;
}
PF_HD void pf_fill_put(float* v, long plane, long i, int C, const PfFill4& r) {
    v[i] = r.v0;
    if (C > 1) v[plane + i] = r.v1;
    if (C > 2) v[2 * plane + i] = r.v2;
    if (C > 3) v[3 * plane + i] = r.v3;
}

// coarse cell (j, i) from the fine level `f` of hf x wf cells
template <class F>
PF_HD void pf_fill_pull_cell(const F& f, int C, int hf, int wf, int j, int i, PfFill4& V, float& S) {
    float s = 0.f, n0 = 0.f, n1 = 0.f, n2 = 0.f, n3 = 0.f;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            // a cell outside the level is read at the nearest one inside and not taken: no load waits for a branch
            const int y = 2 * j + dy < hf ? 2 * j + dy : hf - 1, x = 2 * i + dx < wf ? 2 * i + dx : wf - 1;
            const float w = f.wt(y, x);
            const float v0 = f.val(0, y, x), v1 = C > 1 ? f.val(1, y, x) : 0.f, v2 = C > 2 ? f.val(2, y, x) : 0.f,
                        v3 = C > 3 ? f.val(3, y, x) : 0.f;
            const bool take = (2 * j + dy < hf) & (2 * i + dx < wf) & (w > 0.f);
            s = take ? s + w : s;
            n0 = take ? n0 + w * v0 : n0;
            n1 = take ? n1 + w * v1 : n1;
            n2 = take ? n2 + w * v2 : n2;
            n3 = take ? n3 + w * v3 : n3;
        }
    const bool any = s > 0.f;
    V.v0 = any ? n0 / s : 0.f;
    V.v1 = any && C > 1 ? n1 / s : 0.f;
    V.v2 = any && C > 2 ? n2 / s : 0.f;
    V.v3 = any && C > 3 ? n3 / s : 0.f;
    S = s < 1.f ? s : 1.f;
}
// the two taps of fine coordinate x and the weight of the second
PF_HD void pf_fill_taps(int x, int& a, int& b, float& t) {
    if (x & 1) { a = (x - 1) / 2; b = (x + 1) / 2; t = 0.25f; }
    else { a = x / 2 - 1; b = x / 2; t = 0.75f; }
}
// fine cell (y, x) of the level `f` from the filled coarse level `u` of hc x wc cells (u.val takes a clamped row and a wrapped column)
template <class U, class F>
PF_HD PfFill4 pf_fill_push_cell(const U& u, const F& f, int C, int hc, int wc, int y, int x) {
    // the cell's own value and the taps are all read before the choice between them: no load waits for a branch
    const float w = f.wt(y, x);
    const float v0 = f.val(0, y, x), v1 = C > 1 ? f.val(1, y, x) : 0.f, v2 = C > 2 ? f.val(2, y, x) : 0.f, v3 = C > 3 ? f.val(3, y, x) : 0.f;
    PfFill4 r;
    r.v0 = r.v1 = r.v2 = r.v3 = 0.f;
    int xa, xb, ya, yb;
    float tx, ty;
    pf_fill_taps(x, xa, xb, tx);
    pf_fill_taps(y, ya, yb, ty);
    xa = xa < 0 ? xa + wc : xa;                                  // xa >= -1, xb <= wc: one step is the Python modulo
    xb = xb >= wc ? xb - wc : xb;
    ya = ya < 0 ? 0 : ya;
    yb = yb > hc - 1 ? hc - 1 : yb;
    const bool keep = w >= 1.f, soft = w > 0.f;
#define PF_FILL_UP(c) pf_fill_lerp(pf_fill_lerp(u.val(c, ya, xa), u.val(c, ya, xb), tx), pf_fill_lerp(u.val(c, yb, xa), u.val(c, yb, xb), tx), ty)
#define PF_FILL_MIX(c, v) { const float up = PF_FILL_UP(c); const float mix = pf_fill_lerp(up, v, w); r.v = keep ? v : (soft ? mix : up); }
    PF_FILL_MIX(0, v0)
    if (C > 1) PF_FILL_MIX(1, v1)
    if (C > 2) PF_FILL_MIX(2, v2)
    if (C > 3) PF_FILL_MIX(3, v3)
#undef PF_FILL_MIX
#undef PF_FILL_UP
    return r;
}
// the 1 x 1 level: its value where it has weight, else 0
template <class F>
PF_HD PfFill4 pf_fill_apex_cell(const F& f, int C, bool& empty) {
    const bool known = f.wt(0, 0) > 0.f;
    PfFill4 r;
    r.v0 = known ? f.val(0, 0, 0) : 0.f;
    r.v1 = known && C > 1 ? f.val(1, 0, 0) : 0.f;
    r.v2 = known && C > 2 ? f.val(2, 0, 0) : 0.f;
    r.v3 = known && C > 3 ? f.val(3, 0, 0) : 0.f;
    empty = !known;
    return r;
}

// ---- the level-by-level form: one item of each launch -------------------------------------------------------------------------
struct PfFillPrepArgs { const float* src; const unsigned char* hole; const float* weight; float* w0; int B, C, H, W; };
struct PfFillPullArgs { const float* fine_v; const float* fine_w; float* coarse_v; float* coarse_w; int B, C, hf, wf, hc, wc; };
struct PfFillPushArgs {
    const float* coarse_u; const float* fine_v; const float* fine_w; float* out; unsigned char* empty; int B, C, hf, wf, hc, wc;
};
PF_HD void pf_fill_prepare_pixel(const PfFillPrepArgs& a, long b, long n) {
    const long N = (long)a.H * a.W;
    a.w0[b * N + n] = pf_fill_w0(a.src + b * a.C * N, a.hole + b * N, a.weight ? a.weight + b * N : nullptr, a.C, N, n);
}
PF_HD void pf_fill_pull_item(const PfFillPullArgs& a, long b, long n) {
    const long nf = (long)a.hf * a.wf, nc = (long)a.hc * a.wc;
    PfFillMap f;
    f.v = a.fine_v + b * a.C * nf; f.w = a.fine_w + b * nf; f.width = a.wf; f.plane = nf;
    PfFill4 V;
    float S;
    pf_fill_pull_cell(f, a.C, a.hf, a.wf, (int)(n / a.wc), (int)(n % a.wc), V, S);
    pf_fill_put(a.coarse_v + b * a.C * nc, nc, n, a.C, V);
    a.coarse_w[b * nc + n] = S;
}
// the apex step when coarse_u is null (the fine level is 1 x 1)
PF_HD void pf_fill_push_item(const PfFillPushArgs& a, long b, long n) {
    const long nf = (long)a.hf * a.wf, nc = (long)a.hc * a.wc;
    PfFillMap f;
    f.v = a.fine_v + b * a.C * nf; f.w = a.fine_w + b * nf; f.width = a.wf; f.plane = nf;
    PfFill4 r;
    if (!a.coarse_u) {
        bool empty;
        r = pf_fill_apex_cell(f, a.C, empty);
        if (a.empty) a.empty[b] = empty ? 1 : 0;
    } else {
        PfFillMap u;
        u.v = a.coarse_u + b * a.C * nc; u.w = nullptr; u.width = a.wc; u.plane = nc;
        r = pf_fill_push_cell(u, f, a.C, a.hc, a.wc, (int)(n / a.wf), (int)(n % a.wf));
    }
    pf_fill_put(a.out + b * a.C * nf, nf, n, a.C, r);
}

// ---- the fused form: (a) the pull tile --------------------------------------------------------------------------------------------
// A workgroup of PF_FILL_THREADS owns the level-0 tile at (ty0, tx0), multiples of 32 and 64, and with it the aligned cells
// (ty0 >> k, tx0 >> k) + (32 >> k) x (64 >> k) of the levels k = 1..P: a pull never looks outside its 2 x 2 block, so they nest.
struct PfFillTileMap {                        // level k of the tile in LDS, addressed with the level's own coordinates
    const float* t; int C, oy, ox, tw, cells;
    PF_HD float wt(int y, int x) const { return t[C * cells + (y - oy) * tw + (x - ox)]; }
    PF_HD float val(int c, int y, int x) const { return t[c * cells + (y - oy) * tw + (x - ox)]; }
};
PF_HD int pf_fill_pt_off(int k) { return 5 * ((2048 - (2048 >> (2 * (k - 1)))) / 3); }      // 5 * (512 + 128 + ... ) cells below level k
PF_HD PfFillTileMap pf_fill_tile_map(const float* lds, int C, int ty0, int tx0, int k) {
    PfFillTileMap m;
    m.t = lds + pf_fill_pt_off(k); m.C = C; m.oy = ty0 >> k; m.ox = tx0 >> k; m.tw = PF_FILL_TW >> k;
    m.cells = (PF_FILL_TH >> k) * (PF_FILL_TW >> k);
    return m;
}
// phase k = 1..P of thread tid: the tile's cells of level k, into LDS and into scratch; a barrier follows
PF_HD void pf_fill_pulltile_phase(const PfFillArgs& a, float* lds, long b, int ty0, int tx0, int k, int tid) {
    const int C = a.C, tw = PF_FILL_TW >> k, cells = (PF_FILL_TH >> k) * tw;
    int hf, wf, hc, wc;
    pf_fill_dims(a.H, a.W, k - 1, hf, wf);
    pf_fill_dims(a.H, a.W, k, hc, wc);
    const long nc = (long)hc * wc, off = pf_fill_level_off(a.B, C, a.H, a.W, k);
    float* gv = a.scratch + off + b * C * nc;
    float* gw = a.scratch + off + (long)a.B * C * nc + b * nc;
    float* t = lds + pf_fill_pt_off(k);
    const int oy = ty0 >> k, ox = tx0 >> k;
    for (int cell = tid; cell < cells; cell += PF_FILL_THREADS) {
        const int J = oy + cell / tw, I = ox + cell % tw;
        if (J >= hc || I >= wc) continue;
        PfFill4 V;
        float S;
        if (k == 1) pf_fill_pull_cell(pf_fill_src(a, b), C, hf, wf, J, I, V, S);
        else pf_fill_pull_cell(pf_fill_tile_map(lds, C, ty0, tx0, k - 1), C, hf, wf, J, I, V, S);
        pf_fill_put(t, cells, cell, C, V);
        t[C * cells + cell] = S;
        const long g = (long)J * wc + I;
        pf_fill_put(gv, nc, g, C, V);
        gw[g] = S;
    }
}

// ---- the fused form: (b) the apex ----------------------------------------------------------------------------------------------------
// One workgroup per image.  Level S stays in scratch, the levels S + 1 .. L live in LDS (pf_fill_plan made them fit).
struct PfFillLevel { float* v; float* w; int h, wd; };            // one image's level: values [C][h][wd], weights [h][wd]
PF_HD PfFillLevel pf_fill_apex_level(const PfFillArgs& a, float* lds, long b, int l) {
    PfFillLevel q;
    pf_fill_dims(a.H, a.W, l, q.h, q.wd);
    const long n = (long)q.h * q.wd;
    if (l == a.S) {
        const long off = pf_fill_level_off(a.B, a.C, a.H, a.W, l);
        q.v = a.scratch + off + b * a.C * n;
        q.w = a.scratch + off + (long)a.B * a.C * n + b * n;
    } else {
        q.v = lds + pf_fill_above(a.C, a.H, a.W, a.S, l - 1);
        q.w = q.v + a.C * n;
    }
    return q;
}
PF_HD PfFillMap pf_fill_map_of(const PfFillLevel& q) {
    PfFillMap m;
    m.v = q.v; m.w = q.w; m.width = q.wd; m.plane = (long)q.h * q.wd;
    return m;
}
// The levels are looked up once per workgroup: thread l of the first phase writes tab[l] = pf_fill_apex_level(l) for S <= l <= L
// (a table of PF_FILL_MAX_LEVELS + 1 entries; a barrier follows), so that no later phase walks the pyramid's sizes again.
// level l + 1 from level l (S <= l < L); a barrier follows
PF_HD void pf_fill_apex_pull(const PfFillArgs& a, const PfFillLevel* tab, int l, int tid) {
    const PfFillLevel f = tab[l], c = tab[l + 1];
    const PfFillMap fm = pf_fill_map_of(f);
    const int nc = c.h * c.wd;
    for (int n = tid; n < nc; n += PF_FILL_APEX_THREADS) {
        PfFill4 V;
        float S;
        pf_fill_pull_cell(fm, a.C, f.h, f.wd, n / c.wd, n % c.wd, V, S);
        pf_fill_put(c.v, nc, n, a.C, V);
        c.w[n] = S;
    }
}
// the 1 x 1 level, thread 0; a barrier follows
PF_HD void pf_fill_apex_top(const PfFillArgs& a, const PfFillLevel* tab, long b) {
    const PfFillLevel q = tab[a.L];
    bool empty;
    const PfFill4 r = pf_fill_apex_cell(pf_fill_map_of(q), a.C, empty);
    pf_fill_put(q.v, 1, 0, a.C, r);
    if (a.empty) a.empty[b] = empty ? 1 : 0;
}
// level l, filled in place, from the filled level l + 1 (L > l >= S); a barrier follows
PF_HD void pf_fill_apex_push(const PfFillArgs& a, const PfFillLevel* tab, int l, int tid) {
    const PfFillLevel f = tab[l], c = tab[l + 1];
    const PfFillMap fm = pf_fill_map_of(f), um = pf_fill_map_of(c);
    const int nf = f.h * f.wd;                                   // below 2^30
    for (int n = tid; n < nf; n += PF_FILL_APEX_THREADS) {
        const PfFill4 r = pf_fill_push_cell(um, fm, a.C, c.h, c.wd, n / f.wd, n % f.wd);
        pf_fill_put(f.v, nf, n, a.C, r);
    }
}

// ---- the fused form: (c) the push tile ------------------------------------------------------------------------------------------------
// The workgroup of the level-0 tile rows y0..y1, columns x0..x1 keeps of level l = 1..P the region of rows
// (y0 >> l) - 2 .. (y1 >> l) + 2, cut to the level, and of columns (x0 >> l) - 2 .. (x1 >> l) + 2 modulo W_l (the whole row when
// that many columns exist).  The region of level l + 1 holds both taps of every cell of the region of level l: a tap of column x
// lies in floor((x - 1) / 2) .. floor((x + 1) / 2), which maps -2 .. +2 around the shifted ends into itself, and the columns
// W_l - 2, W_l - 1 left of the seam tap W_(l+1) - 2 .. W_(l+1) (= 0) whether W_l is odd or even, the columns 0, 1 right of it
// W_(l+1) - 1 .. 1.  A cell is found by its own (wrapped) coordinates, never by the position it was asked from, and the position
// is cut to the region, so a fault in this argument would show as a wrong value, not as an access outside the tile's LDS.
struct PfFillRegion { int ylo, ny, xlo, nx, h, w; };
PF_HD PfFillRegion pf_fill_region(int H, int W, int l, int y0, int y1, int x0, int x1) {
    PfFillRegion r;
    pf_fill_dims(H, W, l, r.h, r.w);
    r.ylo = (y0 >> l) - 2;
    r.ylo = r.ylo < 0 ? 0 : r.ylo;
    int yhi = (y1 >> l) + 2;
    yhi = yhi > r.h - 1 ? r.h - 1 : yhi;
    r.ny = yhi - r.ylo + 1;
    r.xlo = (x0 >> l) - 2;
    r.nx = (x1 >> l) + 2 - r.xlo + 1;
    if (r.nx >= r.w) { r.xlo = 0; r.nx = r.w; }
    return r;
}
PF_HD int pf_fill_pu_off(int l) {
    return 4 * (l == 1 ? 0 : (l == 2 ? PF_FILL_R1 : (l == 3 ? PF_FILL_R1 + PF_FILL_R2 : (l == 4 ? PF_FILL_R1 + PF_FILL_R2 + PF_FILL_R3
                : PF_FILL_R1 + PF_FILL_R2 + PF_FILL_R3 + PF_FILL_R4))));
}
struct PfFillRegionMap {
    const float* u; PfFillRegion r;
    PF_HD float val(int c, int y, int x) const {
        int ry = y - r.ylo, rx = x - r.xlo;
        rx = rx < 0 ? rx + r.w : (rx >= r.w ? rx - r.w : rx);
        ry = ry < 0 ? 0 : (ry > r.ny - 1 ? r.ny - 1 : ry);
        rx = rx > r.nx - 1 ? r.nx - 1 : rx;
        return u[c * (r.ny * r.nx) + ry * r.nx + rx];
    }
};
// the level's own coordinates of region cell k
PF_HD void pf_fill_region_cell(const PfFillRegion& r, int k, int& y, int& x) {
    y = r.ylo + k / r.nx;
    x = r.xlo + k % r.nx;
    x = x < 0 ? x + r.w : (x >= r.w ? x - r.w : x);
}
struct PfFillTile { int y0, y1, x0, x1; };
PF_HD PfFillTile pf_fill_tile(int H, int W, int ty0, int tx0) {
    PfFillTile t;
    t.y0 = ty0; t.x0 = tx0;
    t.y1 = ty0 + PF_FILL_TH - 1 < H - 1 ? ty0 + PF_FILL_TH - 1 : H - 1;
    t.x1 = tx0 + PF_FILL_TW - 1 < W - 1 ? tx0 + PF_FILL_TW - 1 : W - 1;
    return t;
}
// phase 1: the region of the filled level P from scratch; a barrier follows
PF_HD void pf_fill_pushtile_load(const PfFillArgs& a, float* lds, long b, int ty0, int tx0, int tid) {
    const PfFillTile t = pf_fill_tile(a.H, a.W, ty0, tx0);
    const PfFillRegion r = pf_fill_region(a.H, a.W, a.P, t.y0, t.y1, t.x0, t.x1);
    const long n = (long)r.h * r.w;
    const float* g = a.scratch + pf_fill_level_off(a.B, a.C, a.H, a.W, a.P) + b * a.C * n;
    float* u = lds + pf_fill_pu_off(a.P);
    const int cells = r.ny * r.nx;
    for (int k = tid; k < cells; k += PF_FILL_THREADS) {
        int y, x;
        pf_fill_region_cell(r, k, y, x);
        const long i = (long)y * r.w + x;
        u[k] = g[i];
        if (a.C > 1) u[cells + k] = g[n + i];
        if (a.C > 2) u[2 * cells + k] = g[2 * n + i];
        if (a.C > 3) u[3 * cells + k] = g[3 * n + i];
    }
}
// phase of level l = P - 1 .. 1: its region, filled, from the stored level and the region above; a barrier follows
PF_HD void pf_fill_pushtile_level(const PfFillArgs& a, float* lds, long b, int ty0, int tx0, int l, int tid) {
    const PfFillTile t = pf_fill_tile(a.H, a.W, ty0, tx0);
    const PfFillRegion r = pf_fill_region(a.H, a.W, l, t.y0, t.y1, t.x0, t.x1);
    PfFillRegionMap um;
    um.r = pf_fill_region(a.H, a.W, l + 1, t.y0, t.y1, t.x0, t.x1);
    um.u = lds + pf_fill_pu_off(l + 1);
    const long n = (long)r.h * r.w, off = pf_fill_level_off(a.B, a.C, a.H, a.W, l);
    PfFillMap f;
    f.v = a.scratch + off + b * a.C * n; f.w = a.scratch + off + (long)a.B * a.C * n + b * n; f.width = r.w; f.plane = n;
    float* u = lds + pf_fill_pu_off(l);
    const int cells = r.ny * r.nx;
    for (int k = tid; k < cells; k += PF_FILL_THREADS) {
        int y, x;
        pf_fill_region_cell(r, k, y, x);
        pf_fill_put(u, cells, k, a.C, pf_fill_push_cell(um, f, a.C, um.r.h, um.r.w, y, x));
    }
}
// the last phase: the tile of out; a wave owns 64 consecutive x of a row
PF_HD void pf_fill_pushtile_out(const PfFillArgs& a, const float* lds, long b, int ty0, int tx0, int tid) {
    const PfFillTile t = pf_fill_tile(a.H, a.W, ty0, tx0);
    PfFillRegionMap um;
    um.r = pf_fill_region(a.H, a.W, 1, t.y0, t.y1, t.x0, t.x1);
    um.u = lds + pf_fill_pu_off(1);
    const PfFillSrc f = pf_fill_src(a, b);
    const long N = (long)a.H * a.W;
    const int x = tx0 + (tid & (PF_FILL_TW - 1));
    if (x > t.x1) return;
    for (int y = ty0 + tid / PF_FILL_TW; y <= t.y1; y += PF_FILL_THREADS / PF_FILL_TW)
        pf_fill_put(a.out + b * a.C * N, N, (long)y * a.W + x, a.C, pf_fill_push_cell(um, f, a.C, um.r.h, um.r.w, y, x));
}

// ---- argument checks shared by the device entries and their host emulation ---------------------------------------------------
static inline bool pf_fill_meet(const void* p, long pb, const void* q, long qb) {
    if (!p || !q) return false;
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + (uintptr_t)qb && b < a + (uintptr_t)pb;
}
static inline bool pf_fill_mis4(const void* p) { return ((uintptr_t)p & 3) != 0; }
// every out[i] against every in[j] and every out[j], j < i
static inline bool pf_fill_overlap(const void* const* out, const long* outb, int n_out, const void* const* in, const long* inb, int n_in) {
    for (int i = 0; i < n_out; ++i) {
        for (int j = 0; j < n_in; ++j) if (pf_fill_meet(out[i], outb[i], in[j], inb[j])) return true;
        for (int j = 0; j < i; ++j) if (pf_fill_meet(out[i], outb[i], out[j], outb[j])) return true;
    }
    return false;
}
static inline int pf_fill_geometry(int B, int C, int H, int W) {
    if (C < 1 || C > 4) return PF_ERR_BAD_ARG;
    if (B < 1 || H < 1 || W < 1 || B > PF_FILL_MAX_GRID || (long)H * W >= (1L << 30)) return PF_ERR_BAD_SHAPE;
    return PF_OK;
}
static inline int pf_fill_levels_of(int H, int W) {
    if (H < 1 || W < 1 || (long)H * W >= (1L << 30)) return PF_ERR_BAD_SHAPE;
    return pf_fill_count_levels(H, W);
}
static inline long pf_fill_bytes_of(int B, int C, int H, int W) {
    const int rc = pf_fill_geometry(B, C, H, W);
    if (rc != PF_OK) return rc;
    int L, P, S;
    pf_fill_plan(C, H, W, L, P, S);
    return 4 * pf_fill_level_off(B, C, H, W, L + 1);
}
static inline int pf_fill_pushpull_check(const float* src, const unsigned char* hole, const float* weight, float* out,
                                         unsigned char* empty, void* scratch, int B, int C, int H, int W, PfFillArgs& a) {
    if (!src || !hole || !out || !scratch) return PF_ERR_BAD_ARG;
    if (pf_fill_mis4(src) || pf_fill_mis4(weight) || pf_fill_mis4(out) || pf_fill_mis4(scratch)) return PF_ERR_BAD_ARG;
    const int rc = pf_fill_geometry(B, C, H, W);
    if (rc != PF_OK) return rc;
    const long N = (long)B * H * W;
    const void* in[3] = {out == src ? nullptr : src, hole, weight};         // out may be exactly src: level 0 reads its own pixel only
    const long inb[3] = {N * C * 4, N, N * 4};
    const void* o[3] = {out, empty, scratch};
    const long ob[3] = {N * C * 4, (long)B, pf_fill_bytes_of(B, C, H, W)};
    if (pf_fill_overlap(o, ob, 3, in, inb, 3)) return PF_ERR_BAD_ARG;
    if (out != src && pf_fill_meet(out, ob[0], src, inb[0])) return PF_ERR_BAD_ARG;
    if (pf_fill_meet(src, inb[0], empty, ob[1]) || pf_fill_meet(src, inb[0], scratch, ob[2])) return PF_ERR_BAD_ARG;
    a.src = src; a.hole = hole; a.weight = weight; a.out = out; a.empty = empty; a.scratch = static_cast<float*>(scratch);
    a.B = B; a.C = C; a.H = H; a.W = W;
    pf_fill_plan(C, H, W, a.L, a.P, a.S);
    return PF_OK;
}
static inline int pf_fill_prepare_check(const float* src, const unsigned char* hole, const float* weight, float* w0, int B, int C,
                                        int H, int W, PfFillPrepArgs& a) {
    if (!src || !hole || !w0 || pf_fill_mis4(src) || pf_fill_mis4(weight) || pf_fill_mis4(w0)) return PF_ERR_BAD_ARG;
    const int rc = pf_fill_geometry(B, C, H, W);
    if (rc != PF_OK) return rc;
    const long N = (long)B * H * W;
    const void* in[3] = {src, hole, weight};
    const long inb[3] = {N * C * 4, N, N * 4};
    const void* o[1] = {w0};
    const long ob[1] = {N * 4};
    if (pf_fill_overlap(o, ob, 1, in, inb, 3)) return PF_ERR_BAD_ARG;
    a.src = src; a.hole = hole; a.weight = weight; a.w0 = w0; a.B = B; a.C = C; a.H = H; a.W = W;
    return PF_OK;
}
static inline int pf_fill_pull_check(const float* fine_v, const float* fine_w, float* coarse_v, float* coarse_w, int B, int C, int hf,
                                     int wf, PfFillPullArgs& a) {
    if (!fine_v || !fine_w || !coarse_v || !coarse_w) return PF_ERR_BAD_ARG;
    if (pf_fill_mis4(fine_v) || pf_fill_mis4(fine_w) || pf_fill_mis4(coarse_v) || pf_fill_mis4(coarse_w)) return PF_ERR_BAD_ARG;
    const int rc = pf_fill_geometry(B, C, hf, wf);
    if (rc != PF_OK) return rc;
    if (hf == 1 && wf == 1) return PF_ERR_BAD_SHAPE;                      // the apex has no level above it
    const int hc = pf_fill_half(hf), wc = pf_fill_half(wf);
    const long nf = (long)B * hf * wf, nc = (long)B * hc * wc;
    const void* in[2] = {fine_v, fine_w};
    const long inb[2] = {nf * C * 4, nf * 4};
    const void* o[2] = {coarse_v, coarse_w};
    const long ob[2] = {nc * C * 4, nc * 4};
    if (pf_fill_overlap(o, ob, 2, in, inb, 2)) return PF_ERR_BAD_ARG;
    a.fine_v = fine_v; a.fine_w = fine_w; a.coarse_v = coarse_v; a.coarse_w = coarse_w;
    a.B = B; a.C = C; a.hf = hf; a.wf = wf; a.hc = hc; a.wc = wc;
    return PF_OK;
}
static inline int pf_fill_push_check(const float* coarse_u, const float* fine_v, const float* fine_w, float* out, unsigned char* empty,
                                     int B, int C, int hf, int wf, PfFillPushArgs& a) {
    if (!fine_v || !fine_w || !out) return PF_ERR_BAD_ARG;
    if (pf_fill_mis4(coarse_u) || pf_fill_mis4(fine_v) || pf_fill_mis4(fine_w) || pf_fill_mis4(out)) return PF_ERR_BAD_ARG;
    const int rc = pf_fill_geometry(B, C, hf, wf);
    if (rc != PF_OK) return rc;
    const bool apex = hf == 1 && wf == 1;
    if (apex != (coarse_u == nullptr) || (empty && !apex)) return PF_ERR_BAD_ARG;      // the apex step, and only it, has no coarse level
    const int hc = pf_fill_half(hf), wc = pf_fill_half(wf);
    const long nf = (long)B * hf * wf, nc = (long)B * hc * wc;
    const void* in[3] = {coarse_u, out == fine_v ? nullptr : fine_v, fine_w};           // in place: a cell reads its own value only
    const long inb[3] = {nc * C * 4, nf * C * 4, nf * 4};
    const void* o[2] = {out, empty};
    const long ob[2] = {nf * C * 4, (long)B};
    if (pf_fill_overlap(o, ob, 2, in, inb, 3)) return PF_ERR_BAD_ARG;
    if (pf_fill_meet(empty, ob[1], fine_v, inb[1])) return PF_ERR_BAD_ARG;
    a.coarse_u = coarse_u; a.fine_v = fine_v; a.fine_w = fine_w; a.out = out; a.empty = empty;
    a.B = B; a.C = C; a.hf = hf; a.wf = wf; a.hc = hc; a.wc = wc;
    return PF_OK;
}
