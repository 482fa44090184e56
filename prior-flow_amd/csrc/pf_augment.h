// Per-pixel functions of the 360-degree training augmentation (include/priorflow_hip.h, pf_augment_360).
//
// What core/utils/augmentor.py:210-316 (FlowAugmentor_360) and core/datasets.py:137-159 do to one sample, restated per pixel:
// torchvision's ColorJitter on its PIL backend (8 bits in and out after every operation), the eraser, the yaw roll, the
// flow's wrap and `valid`.  The same functions compile for the host (tests/emu/pf_emu_augment.cpp).  Built without
// contraction like every unit; the HSV steps follow Pillow's C (fp32 ratios, the last steps in double).
#pragma once
#include "pf_common.h"
#include "pf_elem.h"
#include "../../include/priorflow_hip.h"      // PF_MAX_IMAGES, PF_AUG_ROW_WORDS; checks the definitions against their declarations

// One row of the parameter table: PF_AUG_ROW 32-bit words per sample (factors are fp32 bit patterns).
#define PF_AUG_ROW 32
static_assert(PF_AUG_ROW == PF_AUG_ROW_WORDS, "the row length of pf_augment.h and of the public header");
#define PF_AUG_MODE 0        // bit 0: asymmetric colour (set A -> image 1, set B -> image 2); bit 1: asymmetric roll
#define PF_AUG_NRECT 1       // 0, 1 or 2 eraser rectangles
#define PF_AUG_R1 2          // roll of image 1 and the flow, whole pixels, any sign
#define PF_AUG_R2 3          // roll of image 2 (the symmetric form has r2 == r1)
#define PF_AUG_RECT 4        // 2 x {x0, y0, dx, dy}, before the roll
#define PF_AUG_SET_A 12      // {order[4], brightness, contrast, saturation (fp32), hue shift (0..255)}
#define PF_AUG_SET_B 20
#define PF_AUG_ASYM_COLOUR 1
#define PF_AUG_ASYM_ROLL 2
#define PF_AUG_OP_BRIGHTNESS 0
#define PF_AUG_OP_CONTRAST 1
#define PF_AUG_OP_SATURATION 2
#define PF_AUG_OP_HUE 3
#define PF_AUG_OP_NONE 4     // (and every other value) the step is skipped
// per-sample sums, 64-bit integers: L of set A's image(s), L of set B's image, image 2's three channel sums after the colour step
#define PF_AUG_SUMS 8

struct PfAugSet { int order[4]; float fb, fc, fs; int shift; };
struct PfAugRgb { int r, g, b; };

PF_HD float pf_aug_bits(int w) { union { int i; float f; } v; v.i = w; return v.f; }
PF_HD PfAugSet pf_aug_set(const int* row, int second) {
    const int* p = row + (second ? PF_AUG_SET_B : PF_AUG_SET_A);
    PfAugSet s;
    for (int j = 0; j < 4; ++j) s.order[j] = p[j];
    s.fb = pf_aug_bits(p[4]); s.fc = pf_aug_bits(p[5]); s.fs = pf_aug_bits(p[6]); s.shift = p[7] & 255;
    return s;
}
// which parameter set image `img` (0, 1) of a sample takes, and which L sum its contrast reads
PF_HD int pf_aug_second(const int* row, int img) { return (row[PF_AUG_MODE] & PF_AUG_ASYM_COLOUR) && img == 1; }
// steps of the chain before the contrast step; -1: no contrast step, or one that is the identity (factor 1)
PF_HD int pf_aug_contrast_at(const PfAugSet& s) {
    if (s.fc == 1.0f) return -1;
    for (int j = 0; j < 4; ++j) if (s.order[j] == PF_AUG_OP_CONTRAST) return j;
    return -1;
}
PF_HD int pf_aug_wrap(int x, int W) { x %= W; return x < 0 ? x + W : x; }

// PIL's RGB -> L
PF_HD int pf_aug_luma(const PfAugRgb& c) { return (19595 * c.r + 38470 * c.g + 7471 * c.b + 0x8000) >> 16; }
// Image.blend(degenerate, image, f): deg + f (v - deg) in fp32, clamped to [0, 255], truncated
PF_HD int pf_aug_blend(int deg, int v, float f) {
    const float t = (float)deg + f * (float)(v - deg);
    return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}
PF_HD PfAugRgb pf_aug_blend3(int dr, int dg, int db, const PfAugRgb& c, float f) {
    PfAugRgb o; o.r = pf_aug_blend(dr, c.r, f); o.g = pf_aug_blend(dg, c.g, f); o.b = pf_aug_blend(db, c.b, f);
    return o;
}
// Pillow's 8-bit RGB -> HSV (colorsys in C: fp32 ratios, the sums with double constants, bytes by truncation); returned as
// {h, s, v} in the r, g, b members
PF_HD PfAugRgb pf_aug_rgb_to_hsv(const PfAugRgb& c) {
    const int maxc = c.r > c.g ? (c.r > c.b ? c.r : c.b) : (c.g > c.b ? c.g : c.b);
    const int minc = c.r < c.g ? (c.r < c.b ? c.r : c.b) : (c.g < c.b ? c.g : c.b);
    PfAugRgb o; o.r = 0; o.g = 0; o.b = maxc;
    if (minc == maxc) return o;
    const float cr = (float)(maxc - minc);
    const float s = cr / (float)maxc;
    const float rc = (float)(maxc - c.r) / cr, gc = (float)(maxc - c.g) / cr, bc = (float)(maxc - c.b) / cr;
    float h;
    if (c.r == maxc) h = bc - gc;
    else if (c.g == maxc) h = (float)(2.0 + (double)rc - (double)bc);
    else h = (float)(4.0 + (double)gc - (double)rc);
    const double t = (double)h / 6.0 + 1.0;              // in [5/6, 11/6]
    h = (float)(t - floor(t));                           // fmod(t, 1.0)
    const int uh = (int)((double)h * 255.0), us = (int)((double)s * 255.0);
    o.r = uh > 255 ? 255 : uh; o.g = us > 255 ? 255 : us;
    return o;
}
// Pillow's 8-bit HSV -> RGB: sector floor(6 h / 255), p / q / t rounded to nearest (half up: the arguments are >= 0)
PF_HD int pf_aug_round8(double x) { const int v = (int)floor(x + 0.5); return v > 255 ? 255 : v; }
PF_HD PfAugRgb pf_aug_hsv_to_rgb(int h, int s, int v) {
    PfAugRgb o; o.r = v; o.g = v; o.b = v;
    if (s == 0) return o;
    const double h6 = (double)(float)h * 6.0 / 255.0;
    const int i = (int)floor(h6);
    const float f = (float)(h6 - (double)(float)i);
    const float fs = (float)((double)(float)s / 255.0);
    const double vd = (double)(float)v;
    const int p = pf_aug_round8(vd * (1.0 - (double)fs));
    const int q = pf_aug_round8(vd * (1.0 - (double)fs * (double)f));
    const int t = pf_aug_round8(vd * (1.0 - (double)fs * (1.0 - (double)f)));
    switch (i % 6) {
        case 0: o.g = t; o.b = p; break;
        case 1: o.r = q; o.b = p; break;
        case 2: o.r = p; o.b = t; break;
        case 3: o.r = p; o.g = q; break;
        case 4: o.r = t; o.g = p; break;
        default: o.g = p; o.b = q; break;
    }
    return o;
}
// steps [0, upto) of one ColorJitter draw on one pixel; `mean` is the contrast step's int(mean(L) + 0.5)
PF_HD PfAugRgb pf_aug_chain(PfAugRgb c, const PfAugSet& s, int mean, int upto) {
    for (int j = 0; j < upto; ++j) {
        const int op = s.order[j];
        if (op == PF_AUG_OP_BRIGHTNESS) c = pf_aug_blend3(0, 0, 0, c, s.fb);
        else if (op == PF_AUG_OP_CONTRAST) c = pf_aug_blend3(mean, mean, mean, c, s.fc);
        else if (op == PF_AUG_OP_SATURATION) { const int l = pf_aug_luma(c); c = pf_aug_blend3(l, l, l, c, s.fs); }
        else if (op == PF_AUG_OP_HUE) {
            const PfAugRgb q = pf_aug_rgb_to_hsv(c);
            c = pf_aug_hsv_to_rgb((q.r + s.shift) & 255, q.g, q.b);
        }
    }
    return c;
}
// int(sum / n + 0.5) of ImageStat's mean, in integers
PF_HD int pf_aug_mean(unsigned long long sum, unsigned long long n) { return (int)((2ull * sum + n) / (2ull * n)); }
PF_HD PfAugRgb pf_aug_load(const unsigned char* p) { PfAugRgb c; c.r = p[0]; c.g = p[1]; c.b = p[2]; return c; }

// the flow of one output pixel from its source pixel's (u, v): the wrap at load (core/datasets.py:138), the asymmetric roll's
// u_clip((u + r2) - r1) (augmentor.py:273), valid (datasets.py:158); all fp32, one rounding per step
struct PfAugFlow { float u, v, valid; };
PF_HD PfAugFlow pf_aug_flow(float u, float v, int W, int asym, int r1, int r2) {
    const float Wf = (float)W, half = Wf * 0.5f;
    u = pf_pymod(u + half, Wf) - half;
    if (asym) {
        u = (u + (float)r2) - (float)r1;
        u = pf_pymod(u + half, Wf) - half;
    }
    PfAugFlow o; o.u = u; o.v = v;
    o.valid = (fabsf(u) < 1000.f && fabsf(v) < 1000.f) ? 1.f : 0.f;
    return o;
}
// eraser rectangle k of a sample, clipped at the border (no wrap: augmentor.py:247-251); false when it is empty
PF_HD bool pf_aug_rect(const int* row, int k, int H, int W, int& x0, int& y0, int& w, int& h) {
    if (k >= row[PF_AUG_NRECT] || k >= 2) return false;
    const int* r = row + PF_AUG_RECT + 4 * k;
    x0 = r[0]; y0 = r[1];
    if (x0 < 0 || x0 >= W || y0 < 0 || y0 >= H || r[2] <= 0 || r[3] <= 0) return false;
    w = r[2] < W - x0 ? r[2] : W - x0;
    h = r[3] < H - y0 ? r[3] : H - y0;
    return true;
}

// argument checks shared by the device entry and its host emulation
static inline long pf_augment_scratch_bytes_impl(int B) { return B < 1 ? PF_ERR_BAD_SHAPE : (long)B * PF_AUG_SUMS * 8; }
static inline int pf_augment_check(const void* img1, const void* img2, const void* flow, const void* params, const void* o1,
                                   const void* o2, const void* oflow, const void* ovalid, const void* scratch, long scratch_bytes,
                                   int B, int H, int W) {
    if (!img1 || !img2 || !flow || !params || !o1 || !o2 || !oflow || !ovalid || !scratch) return PF_ERR_BAD_ARG;
    if (o1 == o2 || o1 == oflow || o1 == ovalid || o2 == oflow || o2 == ovalid || oflow == ovalid) return PF_ERR_BAD_ARG;
    if ((uintptr_t)scratch % 8 != 0 || (uintptr_t)params % 4 != 0 || (uintptr_t)flow % 4 != 0) return PF_ERR_BAD_ARG;
    if (B < 1 || B > PF_MAX_IMAGES || H < 2 || W < 2 || (long)H * W >= (1L << 30)) return PF_ERR_BAD_SHAPE;
    if (scratch_bytes < pf_augment_scratch_bytes_impl(B)) return PF_ERR_BAD_ARG;
    return PF_OK;
}
