// Per-element device functions of the non-MFMA kernels (samplers, ERP geometry,
// DCCL lookups, convex upsampling, small direct convolutions).
//
// Each `*_elem(idx, args)` computes ONE output element (or one pixel) and is wrapped by
// a __global__ kernel in pf_elem_kernels.hip.  The same functions compile for the host
// (tests/emu) so that index / wrap / padding logic can be checked against the oracle
// without a GPU; the product only ever runs the device build.
//
// Reference citations are relative to /root/reference/PriOr-RAFT.
#pragma once
#include "pf_common.h"

// ----------------------------------------------------------------------------------------------
// accumulation into gradient buffers: device atomics / omp atomic in the host emulation
#if defined(__HIP_DEVICE_COMPILE__)
#define PF_ATOMIC_ADD(ptr, v) atomicAdd((ptr), (v))
#else
#define PF_ATOMIC_ADD(ptr, v) do { float* pf_p_ = (ptr); const float pf_v_ = (v); _Pragma("omp atomic") *pf_p_ += pf_v_; } while (0)
#endif
// scalar helpers
// ----------------------------------------------------------------------------------------------
// bf16 hi|lo split of one value (the operand format of the PF_PREC_BF16X3 GEMMs): hi = bf16_rne(x), lo = bf16_rne(x - hi).
PF_HD unsigned short pf_bf16_rne(float f) {
    union { float f; unsigned u; } v; v.f = f;
    const unsigned r = v.u + 0x7FFFu + ((v.u >> 16) & 1u);     // round to nearest even (finite inputs)
    return (unsigned short)(r >> 16);
}
PF_HD float pf_bf16_to_f32(unsigned short h) {
    union { float f; unsigned u; } v; v.u = (unsigned)h << 16;
    return v.f;
}
// element (row, ch) of a split twin [rows][lds chunks]{hi[32], lo[32]} (include/priorflow_hip.h, pf_conv_desc)
PF_HD void pf_split_put(void* base, long row, int lds, int ch, float x) {
    unsigned short* o = reinterpret_cast<unsigned short*>(base) + (row * lds + (ch >> 5)) * 64 + (ch & 31);
    const unsigned short hi = pf_bf16_rne(x);
    o[0] = hi;
    o[32] = pf_bf16_rne(x - pf_bf16_to_f32(hi));
}
// fp32 -> IEEE fp16 bits, round to nearest even, overflow to Inf, gradual underflow (v_cvt_f16_f32's result for every input;
// written out so that the host build of this file needs no compiler fp16 type)
PF_HD unsigned short pf_f16_rne(float f) {
    union { float f; unsigned u; } v; v.f = f;
    const unsigned sign = (v.u >> 16) & 0x8000u, a = v.u & 0x7fffffffu;
    if (a >= 0x7f800000u) return (unsigned short)(sign | (a > 0x7f800000u ? 0x7e00u : 0x7c00u));   // NaN / Inf
    if (a >= 0x477ff000u) return (unsigned short)(sign | 0x7c00u);                                  // >= 65520: Inf
    if (a >= 0x38800000u)                                                                           // normal (>= 2^-14)
        return (unsigned short)(sign | ((a + 0x0fffu + ((a >> 13) & 1u) - 0x38000000u) >> 13));
    const int shift = 126 - (int)(a >> 23);                     // subnormal: units of 2^-24
    if (shift > 24) return (unsigned short)sign;
    const unsigned m = (a & 0x7fffffu) | 0x800000u, q = m >> shift, rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1);
    return (unsigned short)(sign | (q + ((rem > half || (rem == half && (q & 1u))) ? 1u : 0u)));
}
// element (row, ch) of an f16 map [rows][lds units]{fp16[64]} (include/priorflow_hip.h, PF_PREC_F16)
PF_HD void pf_f16_put(void* base, long row, int lds, int ch, float x) {
    reinterpret_cast<unsigned short*>(base)[(row * lds + (ch >> 6)) * 64 + (ch & 63)] = pf_f16_rne(x);
}

// Python-style float remainder for b > 0 (`xgrid % W`, core/utils/utils.py:83; ATen: fmod, then +b when
// the signs differ), bit for bit, without the device's (long, loop-based) fmodf:
//   0 <= a < b            -> a                       (fmod is the identity)
//   -b < a < 0            -> a + b, ROUNDED          (ATen adds b to fmod = a; a tiny negative gives exactly b)
//   otherwise             -> a - b*floor(a/b): q from a*(1/b) can be off by one, r = fma(-q, b, a) is exact
//                            (for |a| >= b the true remainder lies on a's own ulp grid), one correction step.
// NaN / +-inf propagate to NaN like fmod.  b is an image width (an integer <= 2^20) here.
PF_HD float pf_pymod(float a, float b) {
    if (a >= 0.f && a < b) return a;
    if (a < 0.f && a > -b) return a + b;
    const float q = floorf(a * (1.f / b));
    float r = fmaf(-q, b, a);
    if (r < 0.f) r += b;
    else if (r >= b) r -= b;
    return r == 0.f ? copysignf(0.f, a) : r;       // fmod keeps the dividend's sign on an exact multiple
}

// pixel -> [-1,1] -> pixel round trip of `2x/(W-1)-1` (core/utils/utils.py:85-86) followed
// by grid_sample(align_corners=True)'s unnormalise, each step rounded to fp32.
PF_HD float pf_roundtrip(float p, int size) {
    const float s = (float)(size - 1);
    float pn = (2.f * p) / s;
    pn = pn - 1.f;
    return (pn + 1.f) * (s * 0.5f);
}

struct PfTaps {          // 4 bilinear taps of a zero-padded sample
    int idx[4];          // y*W+x (clamped into range; weight is 0 when out of bounds)
    float w[4];          // nw, ne, sw, se
};

// Zero-padded bilinear taps at pixel coords (x,y) of an H x W map
// (F.grid_sample bilinear / zeros / align_corners=True after the callers' normalisation).
PF_HD PfTaps pf_taps0(float x, float y, int H, int W) {
    PfTaps t;
    const float ix = pf_roundtrip(x, W), iy = pf_roundtrip(y, H);
    const float fx = floorf(ix), fy = floorf(iy);
    const float wx = ix - fx, wy = iy - fy;
    const float ex = 1.f - wx, ey = 1.f - wy;
    // NaN / huge coordinates: every comparison below is false -> all taps out of bounds
    const bool xin0 = (fx >= 0.f) && (fx <= (float)(W - 1));
    const bool xin1 = (fx >= -1.f) && (fx <= (float)(W - 2));
    const bool yin0 = (fy >= 0.f) && (fy <= (float)(H - 1));
    const bool yin1 = (fy >= -1.f) && (fy <= (float)(H - 2));
    const int x0 = xin0 ? (int)fx : 0, x1 = xin1 ? (int)fx + 1 : 0;
    const int y0 = yin0 ? (int)fy : 0, y1 = yin1 ? (int)fy + 1 : 0;
    t.idx[0] = y0 * W + x0; t.w[0] = (xin0 && yin0) ? ey * ex : 0.f;
    t.idx[1] = y0 * W + x1; t.w[1] = (xin1 && yin0) ? ey * wx : 0.f;
    t.idx[2] = y1 * W + x0; t.w[2] = (xin0 && yin1) ? wy * ex : 0.f;
    t.idx[3] = y1 * W + x1; t.w[3] = (xin1 && yin1) ? wy * wx : 0.f;
    return t;
}

PF_HD float pf_apply(const PfTaps& t, const float* img) {
    float acc = img[t.idx[0]] * t.w[0];
    acc = acc + img[t.idx[1]] * t.w[1];
    acc = acc + img[t.idx[2]] * t.w[2];
    acc = acc + img[t.idx[3]] * t.w[3];
    return acc;
}
// same, strided (channel-last maps: element (pixel, c) at img[pixel*ld + c])
PF_HD float pf_apply_ld(const PfTaps& t, const float* img, long ld) {
    float acc = img[(long)t.idx[0] * ld] * t.w[0];
    acc = acc + img[(long)t.idx[1] * ld] * t.w[1];
    acc = acc + img[(long)t.idx[2] * ld] * t.w[2];
    acc = acc + img[(long)t.idx[3] * ld] * t.w[3];
    return acc;
}

// Paired form of the zero-padded taps for PLANAR maps: the two x-corners of a bilinear sample are
// adjacent floats, so a sample is two 8-byte loads (rows y0, y1) instead of four 4-byte gathers.
// The pair starts at column xb = clamp(floor(x), 0, W-2), always inside the row; the corner values
// are picked out of it (x0 = W-1 sits in the pair's second slot, x1 = 0 in its first).  Weights,
// rows and the order of the four products are those of pf_taps0 / pf_apply, so results are identical.
// The DCCL lookup is bound by the number of gather instructions (16 per tap before, 8 now).
struct PfPair { float a, b; };
struct PfQuad { float a, b, c, d; };
PF_HD PfQuad pf_load4(const float* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef float pf_f4u __attribute__((ext_vector_type(4), aligned(4)));     // dword-aligned 16-byte load
    const pf_f4u v = *reinterpret_cast<const pf_f4u*>(p);
    return PfQuad{v.x, v.y, v.z, v.w};
#else
    return PfQuad{p[0], p[1], p[2], p[3]};
#endif
}
PF_HD PfPair pf_load2(const float* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef float pf_f2u __attribute__((ext_vector_type(2), aligned(4)));     // dword-aligned 8-byte load
    const pf_f2u v = *reinterpret_cast<const pf_f2u*>(p);
    return PfPair{v.x, v.y};
#else
    return PfPair{p[0], p[1]};
#endif
}
struct PfTaps2 {
    int r0, r1;          // y0*W + xb, y1*W + xb
    bool s0hi, s1lo;     // x0 value = second slot of the pair / x1 value = first slot
    float w[4];          // nw, ne, sw, se (0 when out of bounds)
};
PF_HD PfTaps2 pf_taps0v(float x, float y, int H, int W) {      // W >= 2
    PfTaps2 t;
    const float ix = pf_roundtrip(x, W), iy = pf_roundtrip(y, H);
    const float fx = floorf(ix), fy = floorf(iy);
    const float wx = ix - fx, wy = iy - fy;
    const float ex = 1.f - wx, ey = 1.f - wy;
    const bool xin0 = (fx >= 0.f) && (fx <= (float)(W - 1));
    const bool xin1 = (fx >= -1.f) && (fx <= (float)(W - 2));
    const bool yin0 = (fy >= 0.f) && (fy <= (float)(H - 1));
    const bool yin1 = (fy >= -1.f) && (fy <= (float)(H - 2));
    // NaN / huge coordinates: every comparison is false -> xb = 0, all weights 0
    const int xb = (fx >= 0.f) ? ((fx <= (float)(W - 2)) ? (int)fx : W - 2) : 0;
    const int y0 = yin0 ? (int)fy : 0, y1 = yin1 ? (int)fy + 1 : 0;
    t.r0 = y0 * W + xb; t.r1 = y1 * W + xb;
    t.s0hi = fx == (float)(W - 1);
    t.s1lo = fx == -1.f;
    t.w[0] = (xin0 && yin0) ? ey * ex : 0.f;
    t.w[1] = (xin1 && yin0) ? ey * wx : 0.f;
    t.w[2] = (xin0 && yin1) ? wy * ex : 0.f;
    t.w[3] = (xin1 && yin1) ? wy * wx : 0.f;
    return t;
}
PF_HD float pf_apply_pairs(const PfTaps2& t, const PfPair p0, const PfPair p1) {
    float acc = (t.s0hi ? p0.b : p0.a) * t.w[0];
    acc = acc + (t.s1lo ? p0.a : p0.b) * t.w[1];
    acc = acc + (t.s0hi ? p1.b : p1.a) * t.w[2];
    acc = acc + (t.s1lo ? p1.a : p1.b) * t.w[3];
    return acc;
}
PF_HD float pf_apply_v(const PfTaps2& t, const float* img) {
    const PfPair p0 = pf_load2(img + t.r0), p1 = pf_load2(img + t.r1);
    float acc = (t.s0hi ? p0.b : p0.a) * t.w[0];
    acc = acc + (t.s1lo ? p0.a : p0.b) * t.w[1];
    acc = acc + (t.s0hi ? p1.b : p1.a) * t.w[2];
    acc = acc + (t.s1lo ? p1.a : p1.b) * t.w[3];
    return acc;
}

// True-wrap (x) / clamp (y) bilinear taps (core/utils/my_cycle_sample.py:31-60).
struct PfWrapTaps { int ia, ib, ic, id; float wa, wb, wc, wd; };
PF_HD PfWrapTaps pf_wraptaps(float gx, float gy, int H, int W) {
    PfWrapTaps t;
    gx = pf_pymod(gx, (float)W);
    float fx = floorf(gx), fy = floorf(gy);
    const float xw = gx - fx, yw = gy - fy;
    // keep the integer conversion defined for NaN / huge values
    if (!(fx >= 0.f && fx <= (float)W)) fx = 0.f;
    if (!(fy >= -1.0e6f)) fy = -1.0e6f;
    if (!(fy <= 1.0e6f)) fy = 1.0e6f;
    int x0 = (int)fx, y0 = (int)fy;
    int x1 = x0 + 1, y1 = y0 + 1;
    x0 = x0 % W; x1 = x1 % W;                      // x0 >= 0 here
    y0 = y0 < 0 ? 0 : (y0 > H - 1 ? H - 1 : y0);
    y1 = y1 < 0 ? 0 : (y1 > H - 1 ? H - 1 : y1);
    t.ia = y0 * W + x0; t.ib = y1 * W + x0; t.ic = y0 * W + x1; t.id = y1 * W + x1;
    t.wa = (1.f - xw) * (1.f - yw);
    t.wb = (1.f - xw) * yw;
    t.wc = xw * (1.f - yw);
    t.wd = xw * yw;
    return t;
}
PF_HD float pf_wrapmix(const PfWrapTaps& t, float a, float b, float c, float d) {
    float acc = t.wa * a + t.wb * b;
    acc = acc + t.wc * c;
    acc = acc + t.wd * d;
    return acc;
}
// seam un-wrapping of the m-channel (core/utils/my_cycle_sample.py:82-97)
PF_HD float pf_unwrap_m(float anchor, float v, float W) {
    float t = (v - anchor) + W * 0.5f;
    t = pf_pymod(t, W);
    return (anchor + t) - W * 0.5f;
}

// ----------------------------------------------------------------------------------------------
// K8: sample grid  (core/utils/projection_prim_ortho.py:432-443 and helpers)
// ----------------------------------------------------------------------------------------------
struct PfGridArgs { float* grid; int H, W; float R[9]; };
PF_HD float pf_nudge(float t) {              // diverge_zero, :69-74
    const float eps = 1e-6f;
    const float sgn = (t > 0.f) ? 1.f : ((t < 0.f) ? -1.f : 0.f);
    return (fabsf(t) < eps) ? t + sgn * eps : t;
}
PF_HD void pf_sample_grid_elem(long idx, const PfGridArgs& a) {
    const float PI = 3.14159274101257324f;       // float32(np.pi)
    const float TWO_PI = 6.28318548202514648f;   // float32(2*np.pi)
    const int m = (int)(idx % a.W), n = (int)(idx / a.W);
    float u = ((float)m + 0.5f) / (float)a.W;
    float theta = ((u - 0.5f) * 2.f) * PI;
    float v = ((float)n + 0.5f) / (float)a.H;
    float phi = (0.5f - v) * PI;
    const float cp = cosf(phi);
    const float x = cp * cosf(theta), y = cp * sinf(theta), z = sinf(phi);
    const float* R = a.R;
    float xr = R[0] * x + R[1] * y; xr = xr + R[2] * z;
    float yr = R[3] * x + R[4] * y; yr = yr + R[5] * z;
    float zr = R[6] * x + R[7] * y; zr = zr + R[8] * z;
    const float phi2 = asinf(zr);
    const float theta2 = atan2f(pf_nudge(yr), pf_nudge(xr));
    float m2 = theta2 / TWO_PI + 0.5f;
    m2 = m2 * (float)a.W - 0.5f;
    float n2 = 0.5f - phi2 / PI;
    n2 = n2 * (float)a.H - 0.5f;
    const long hw = (long)a.H * a.W;
    a.grid[idx] = m2;
    a.grid[hw + idx] = n2;
}

// ----------------------------------------------------------------------------------------------
// K7: img_rotate, NCHW (core/utils/projection_prim_ortho.py:507-514, :119-135)
// ----------------------------------------------------------------------------------------------
struct PfImgRotArgs { const float* img; const float* grid; float* out; int B, C, H, W; };
PF_HD void pf_img_rotate_elem(long idx, const PfImgRotArgs& a) {
    const long hw = (long)a.H * a.W;
    const long pix = idx % hw;
    const long bc = idx / hw;
    const float gx = pf_pymod(a.grid[pix], (float)a.W);
    const float gy = a.grid[hw + pix];
    const PfTaps t = pf_taps0(gx, gy, a.H, a.W);
    a.out[idx] = pf_apply(t, a.img + bc * hw);
}

// ----------------------------------------------------------------------------------------------
// input normalisation 2 * (image / 255.0) - 1.0 of both images (core/prior_raft.py:121-122), written straight into the
// encoders' batches: image1 -> f1 and c1 (feature and context batch), image2 -> f2
// ----------------------------------------------------------------------------------------------
struct PfNormImgArgs { const float* image1; const float* image2; float* f1; float* f2; float* c1; };
PF_HD float pf_norm255(float v) { return 2.f * (v / 255.0f) - 1.0f; }
PF_HD void pf_normalise_images_elem(long idx, const PfNormImgArgs& a) {
    const float v1 = pf_norm255(a.image1[idx]);
    a.f1[idx] = v1;
    if (a.c1) a.c1[idx] = v1;
    a.f2[idx] = pf_norm255(a.image2[idx]);
}

// ----------------------------------------------------------------------------------------------
// The whole input stage in one pass over the pixels (round 6; core/prior_raft.py:121-127): normalise both images and resample
// them into view B, written straight into the encoders' batches
//     f = [im1 | im2 | im1_B | im2_B]   ([4B,3,H,W])        c = [im1 | im1_B]   ([2B,3,H,W], optional)
// A rotated value is sum_q w_q * norm(raw[tap q]): the values pf_img_rotate reads from the normalised image, the same products
// in the same order -- bit-identical to pf_normalise_images + pf_img_rotate (+ the copy of im1_B into c) --, one launch instead of
// three at the head of every forward, where nothing else runs.
// ----------------------------------------------------------------------------------------------
struct PfPrepImgArgs { const float* image1; const float* image2; const float* grid; float* f; float* c; int B, H, W; };
PF_HD void pf_prepare_images_elem(long idx, const PfPrepImgArgs& a) {   // idx over B*3*H*W: one plane position of both images
    const long hw = (long)a.H * a.W;
    const long plane = (idx / hw) * hw;
    long pix = idx % hw;
    // 64 consecutive indices = an 8 x 8 tile of pixels, not 64 pixels of a row: view B is view A turned by 90 degrees, a row
    // segment of B is a column-like curve in A -- up to 64 cache lines per gather instruction, the whole launch bound by the
    // texture cache's tag rate (31 us) --, while an 8 x 8 tile samples an ~8 x 8 region (which thread takes which pixel
    // changes nothing in the results)
    // (8 x 8: 24 us; 4 x 16 and 2 x 32: 27 us; 16 x 4: 34 us; rows: 31 us -- profiles/r6_ab_head_of_forward.txt)
    if (!((a.H | a.W) & 7)) {
        const long tile = pix >> 6;
        const int in = (int)(pix & 63), tpr = a.W >> 3;
        pix = ((tile / tpr) * 8 + (in >> 3)) * a.W + (tile % tpr) * 8 + (in & 7);
    }
    const float gx = pf_pymod(a.grid[pix], (float)a.W);
    const float gy = a.grid[hw + pix];
    const PfTaps t = pf_taps0(gx, gy, a.H, a.W);
    const long img = (long)a.B * 3 * hw;            // elements of one batch of B three-channel images
    const float* p1 = a.image1 + plane;
    const float* p2 = a.image2 + plane;
    // the ten loads first, then the arithmetic, then the six stores (a load behind a possibly aliasing store would wait for it)
    const float o1 = p1[pix], o2 = p2[pix];
    float t1[4], t2[4];
    for (int q = 0; q < 4; ++q) { t1[q] = p1[t.idx[q]]; t2[q] = p2[t.idx[q]]; }
    float r1 = pf_norm255(t1[0]) * t.w[0], r2 = pf_norm255(t2[0]) * t.w[0];      // pf_apply's products and order
    for (int q = 1; q < 4; ++q) { r1 = r1 + pf_norm255(t1[q]) * t.w[q]; r2 = r2 + pf_norm255(t2[q]) * t.w[q]; }
    const float v1 = pf_norm255(o1), v2 = pf_norm255(o2);
    const long o = plane + pix;
    a.f[o] = v1;
    a.f[img + o] = v2;
    a.f[2 * img + o] = r1;
    a.f[3 * img + o] = r2;
    if (a.c) { a.c[o] = v1; a.c[img + o] = r1; }
}

// The input stage of ONE frame (video streams, prior-flow_amd/video.py): out = [im | im_B] ([2B,3,H,W]) -- the image1 half of
// pf_prepare_images, the same pixel order, taps, products and sums: bit-identical to img_c of a pf_prepare_images launch.
struct PfPrepFrameArgs { const float* image; const float* grid; float* out; int B, H, W; };
PF_HD void pf_prepare_frame_elem(long idx, const PfPrepFrameArgs& a) {   // idx over B*3*H*W
    const long hw = (long)a.H * a.W;
    const long plane = (idx / hw) * hw;
    long pix = idx % hw;
    if (!((a.H | a.W) & 7)) {                       // 8 x 8 pixel tiles (pf_prepare_images_elem)
        const long tile = pix >> 6;
        const int in = (int)(pix & 63), tpr = a.W >> 3;
        pix = ((tile / tpr) * 8 + (in >> 3)) * a.W + (tile % tpr) * 8 + (in & 7);
    }
    const float gx = pf_pymod(a.grid[pix], (float)a.W);
    const float gy = a.grid[hw + pix];
    const PfTaps t = pf_taps0(gx, gy, a.H, a.W);
    const long img = (long)a.B * 3 * hw;
    const float* p1 = a.image + plane;
    const float o1 = p1[pix];
    float t1[4];
    for (int q = 0; q < 4; ++q) t1[q] = p1[t.idx[q]];
    float r1 = pf_norm255(t1[0]) * t.w[0];
    for (int q = 1; q < 4; ++q) r1 = r1 + pf_norm255(t1[q]) * t.w[q];
    const long o = plane + pix;
    a.out[o] = pf_norm255(o1);
    a.out[img + o] = r1;
}

// ----------------------------------------------------------------------------------------------
// flow = coords1 - coords0, scattered to planar + up to two channel-last destinations
// (core/prior_raft.py:172,177; coords_grid core/utils/utils.py:98-101)
// ----------------------------------------------------------------------------------------------
struct PfDst { float* ptr; int ld; int c_off; };     // channel-last [B*N][ld] destination slice
struct PfFlowPrepArgs { const float* coords1; float* flow; PfDst d0, d1; int B, H, W; };
PF_HD void pf_store_dst2(const PfDst& d, long row, float u, float v) {
    if (d.ptr) { d.ptr[row * d.ld + d.c_off] = u; d.ptr[row * d.ld + d.c_off + 1] = v; }
}
PF_HD void pf_flow_prep_elem(long idx, const PfFlowPrepArgs& a) {   // idx over B*N
    const long N = (long)a.H * a.W;
    const long b = idx / N, n = idx % N;
    const float x = (float)(n % a.W), y = (float)(n / a.W);
    const float u = a.coords1[(b * 2 + 0) * N + n] - x;
    const float v = a.coords1[(b * 2 + 1) * N + n] - y;
    if (a.flow) { a.flow[(b * 2 + 0) * N + n] = u; a.flow[(b * 2 + 1) * N + n] = v; }
    pf_store_dst2(a.d0, idx, u, v);
    pf_store_dst2(a.d1, idx, u, v);
}

// ----------------------------------------------------------------------------------------------
// K6: flo_rotate (core/utils/projection_prim_ortho.py:531-546, :200-218, :234-244;
//     core/utils/my_cycle_sample.py:6-97)
// ----------------------------------------------------------------------------------------------
struct PfFloRotArgs {
    const float* flow;       // planar [B,2,N]
    const float* g_w2c;      // [2,N]
    const float* g_c2w;      // [2,N]
    float* out;              // planar [B,2,N] (may be null)
    PfDst d0, d1;
    int B, H, W;
};
// camera-frame flow F at pixel p of batch b
PF_HD void pf_flow_c_at(const PfFloRotArgs& a, long b, int p, float& f0, float& f1) {
    const long N = (long)a.H * a.W;
    const float Wf = (float)a.W;
    const float px = (float)(p % a.W), py = (float)(p / a.W);
    float ex = (px + a.flow[(b * 2 + 0) * N + p]) + 0.5f;
    ex = pf_pymod(ex, Wf) - 0.5f;
    float ey = py + a.flow[(b * 2 + 1) * N + p];
    ey = fminf(fmaxf(ey, -0.5f), (float)a.H - 0.5f);
    const PfWrapTaps t = pf_wraptaps(ex, ey, a.H, a.W);
    const float* g0 = a.g_w2c;
    const float* g1 = a.g_w2c + N;
    const float a0 = g0[t.ia];
    const float e0 = pf_wrapmix(t, a0, pf_unwrap_m(a0, g0[t.ib], Wf), pf_unwrap_m(a0, g0[t.ic], Wf),
                                pf_unwrap_m(a0, g0[t.id], Wf));
    const float e1 = pf_wrapmix(t, g1[t.ia], g1[t.ib], g1[t.ic], g1[t.id]);
    f0 = e0 - g0[p];
    f0 = pf_pymod(f0 + Wf * 0.5f, Wf) - Wf * 0.5f;     // u_clip
    f1 = e1 - g1[p];
}
PF_HD void pf_flo_rotate_elem(long idx, const PfFloRotArgs& a) {  // idx over B*N
    const long N = (long)a.H * a.W;
    const long b = idx / N, n = idx % N;
    const PfWrapTaps t = pf_wraptaps(a.g_c2w[n], a.g_c2w[N + n], a.H, a.W);
    float a0, a1, b0, b1, c0, c1, d0, d1;
    pf_flow_c_at(a, b, t.ia, a0, a1);
    pf_flow_c_at(a, b, t.ib, b0, b1);
    pf_flow_c_at(a, b, t.ic, c0, c1);
    pf_flow_c_at(a, b, t.id, d0, d1);
    const float u = pf_wrapmix(t, a0, b0, c0, d0);
    const float v = pf_wrapmix(t, a1, b1, c1, d1);
    if (a.out) { a.out[(b * 2 + 0) * N + n] = u; a.out[(b * 2 + 1) * N + n] = v; }
    pf_store_dst2(a.d0, idx, u, v);
    pf_store_dst2(a.d1, idx, u, v);
}

// ----------------------------------------------------------------------------------------------
// K3 + K4(a,b): own-view and raw cross-view lookups (core/corr.py:113-137)
// ----------------------------------------------------------------------------------------------
struct PfLookupArgs {
    const float* coords;            // planar [B,2,N]
    const float* own[PF_CORR_LEVELS];    // level i: [B*N][H_i*W_i]
    const float* other[PF_CORR_LEVELS];
    const float* g_w2c;             // [2,N]
    const float* g_il;              // optional: the same grid interleaved [N][2] (x, y per pixel), or null
    float* own_out;                 // channel-last [B*N][ld]
    float* raw_out;                 // channel-last [B*N][ld]
    int B, H, W, ld;
};
// One call = PF_LOOKUP_TPT consecutive taps (same level, same slow index a): their gather chains
// (coords -> grid taps -> other-volume taps) are independent, so the loads of all of them are in
// flight together.  Timing-only ablations (round 1; profiles/microbench_lookup.py is the harness) showed the kernel bound by the
// NUMBER of gather instructions, cache-resident ones included (no own-window loads -7 us, no grid loads -9 us,
// no other-volume loads -4 us, no stores -3 us of 32 us).  Consecutive taps of a column share a row (the lower
// row of tap j is the upper row of tap j+1), so a row pair is loaded once and reused when its ADDRESS matches --
// same address, same value: results are bit-identical to per-tap loads.  Own window and the two grid components:
// 4 loads per 3 taps instead of 6 each.  Measured in one call (round-1 A/B): 32.8 us without
// reuse, 27.4 us with it at 3 taps per call, 43 us at 9 taps per call (a whole column: too few, too fat threads).
#ifndef PF_LOOKUP_TPT
#define PF_LOOKUP_TPT 3
#endif
PF_HD void pf_lookup_elem(long idx, const PfLookupArgs& a) {  // idx over B*N*(324/TPT)
    const long N = (long)a.H * a.W;
    const int per_row = PF_CORR_CH / PF_LOOKUP_TPT;
    const int k0 = (int)(idx % per_row) * PF_LOOKUP_TPT;
    const long row = idx / per_row;                    // b*N + n
    const long b = row / N, n = row % N;
    const int lvl = k0 / PF_TAPS, tap0 = k0 % PF_TAPS;
    const int ta = tap0 / 9, tb0 = tap0 % 9;           // slow axis a offsets x (core/corr.py:120-126)
    const int Hl = a.H >> lvl, Wl = a.W >> lvl;
    const float inv = 1.f / (float)(1 << lvl);         // coords / 2**i : exact
    const float cx = a.coords[(b * 2 + 0) * N + n] * inv + (float)(ta - PF_CORR_RADIUS);
    const float cy0 = a.coords[(b * 2 + 1) * N + n] * inv;
    const long lsz = (long)Hl * Wl;
    const float* own = a.own[lvl] + row * lsz;
    const float* oth = a.other[lvl] + row * lsz;
    // own view: x wrapped mod W_i, zero padded.  Cross view: level-i coordinates index the LEVEL-0
    // grid (core/corr.py:132-133), and the result indexes row n of the OTHER branch's volume (:135-136)
    const float xo = pf_pymod(cx, (float)Wl), xg = pf_pymod(cx, (float)a.W);
    float gx[PF_LOOKUP_TPT], gy[PF_LOOKUP_TPT], vo[PF_LOOKUP_TPT];
    int ro = -1, rg = -1;                              // addresses of the row pairs carried from the previous tap
    PfPair po = {0.f, 0.f}, pgx = {0.f, 0.f}, pgy = {0.f, 0.f};
    for (int j = 0; j < PF_LOOKUP_TPT; ++j) {
        const float cy = cy0 + (float)(tb0 + j - PF_CORR_RADIUS);
        const PfTaps2 t = pf_taps0v(xo, cy, Hl, Wl);
#ifdef PF_ABL_NO_OWN          // timing-only ablations; never defined in the product build
        vo[j] = t.w[0] + cy;
#else
        {
            const PfPair p0 = (t.r0 == ro) ? po : pf_load2(own + t.r0);
            const PfPair p1 = pf_load2(own + t.r1);
            vo[j] = pf_apply_pairs(t, p0, p1);
            ro = t.r1; po = p1;
        }
#endif
        const PfTaps2 tg = pf_taps0v(xg, cy, a.H, a.W);
#ifdef PF_ABL_NO_GRID
        gx[j] = xg + tg.w[0]; gy[j] = cy + tg.w[1];
#else
        {
            const bool hit = tg.r0 == rg;
            PfPair x0 = pgx, y0 = pgy, x1, y1;
            if (a.g_il) {
                // interleaved grid: the row pair of BOTH components is one 16-byte load {x(xb), y(xb), x(xb+1), y(xb+1)}
                if (!hit) { const PfQuad q = pf_load4(a.g_il + 2 * (long)tg.r0); x0 = PfPair{q.a, q.c}; y0 = PfPair{q.b, q.d}; }
                const PfQuad q = pf_load4(a.g_il + 2 * (long)tg.r1);
                x1 = PfPair{q.a, q.c}; y1 = PfPair{q.b, q.d};
            } else {
                if (!hit) { x0 = pf_load2(a.g_w2c + tg.r0); y0 = pf_load2(a.g_w2c + N + tg.r0); }
                x1 = pf_load2(a.g_w2c + tg.r1); y1 = pf_load2(a.g_w2c + N + tg.r1);
            }
            gx[j] = pf_apply_pairs(tg, x0, x1);
            gy[j] = pf_apply_pairs(tg, y0, y1);
            rg = tg.r1; pgx = x1; pgy = y1;
        }
#endif
    }
    for (int j = 0; j < PF_LOOKUP_TPT; ++j) {
        const PfTaps2 t = pf_taps0v(pf_pymod(gx[j], (float)Wl), gy[j], Hl, Wl);
#ifndef PF_ABL_NO_STORE
        a.own_out[row * a.ld + k0 + j] = vo[j];
#endif
#ifdef PF_ABL_NO_OTH
        a.raw_out[row * a.ld + k0 + j] = t.w[0] + t.w[3] + vo[j];
#elif defined(PF_ABL_NO_STORE)
        if (pf_apply_v(t, oth) + vo[j] == 123.456f) a.raw_out[row * a.ld + k0 + j] = 1.f;
#else
        a.raw_out[row * a.ld + k0 + j] = pf_apply_v(t, oth);
#endif
    }
}

// ----------------------------------------------------------------------------------------------
// alternate_corr: the same two lookups without the correlation volumes (AlternateCorrBlock, core/corr.py:64-91).
// Pooling is linear, so level i of the pyramid at (n, p) is <f1[n], P_i(f2)[p]> / sqrt(C), P_i = the 2x2 floor mean of
// f2 applied i times (pf_feature_pyramid).  Each bilinear corner is one C-long dot product computed at lookup time.
// ----------------------------------------------------------------------------------------------
struct PfFeatPoolArgs {
    const float* in;                // channel-last [B*H*W][C]
    float* out;                     // channel-last [B*(H/2)*(W/2)][C]
    int B, H, W, C;
};
PF_HD void pf_feat_pool_elem(long idx, const PfFeatPoolArgs& a) {     // idx over B*(H/2)*(W/2)*(C/4)
    const int C4 = a.C / 4, Ho = a.H >> 1, Wo = a.W >> 1;
    const long c = (idx % C4) * 4;
    const long p = idx / C4;
    const long b = p / ((long)Ho * Wo), q = p % ((long)Ho * Wo);
    const long y = q / Wo, x = q % Wo;
    const float* r0 = a.in + ((b * a.H + 2 * y) * a.W + 2 * x) * a.C + c;   // (2y, 2x); odd sizes drop the last row / column
    const float* r2 = r0 + (long)a.W * a.C;
    float* o = a.out + p * a.C + c;
    for (int j = 0; j < 4; ++j) o[j] = (((r0[j] + r0[a.C + j]) + r2[j]) + r2[a.C + j]) * 0.25f;
}

struct PfLookupFeatArgs {
    const float* coords;                    // planar [B,2,N]
    const float* f1_own;                    // channel-last [B*N][C]
    const float* f2_own[PF_CORR_LEVELS];    // level i: channel-last [B*N_i][C] (level 0: f2 itself)
    const float* f1_oth;
    const float* f2_oth[PF_CORR_LEVELS];
    const float* g_w2c;                     // [2,N]
    float* own_out;                         // channel-last [B*N][ld]
    float* raw_out;
    int* path_counts;                       // optional [2]: (tile, level, view) units on the tile / pixel path (device kernel only)
    int B, H, W, C, ld;
    float scale;                            // 1 / sqrt(C)
};
PF_HD float pf_feat_dot(const float* x, const float* y, int C) {
    float s = 0.f;
    for (int c = 0; c < C; ++c) s = s + x[c] * y[c];
    return s;
}
// element index of the four corners of a zero-padded bilinear sample (the picks of pf_apply_pairs), -1 where the weight is 0
PF_HD void pf_taps2_corners(const PfTaps2& t, int (&e)[4]) {
    e[0] = t.w[0] != 0.f ? t.r0 + (t.s0hi ? 1 : 0) : -1;
    e[1] = t.w[1] != 0.f ? t.r0 + (t.s1lo ? 0 : 1) : -1;
    e[2] = t.w[2] != 0.f ? t.r1 + (t.s0hi ? 1 : 0) : -1;
    e[3] = t.w[3] != 0.f ? t.r1 + (t.s1lo ? 0 : 1) : -1;
}
// bilinear sample of the level volume row <f1, f2l[.]> * scale; corners with weight 0 contribute 0 (the volume is finite)
PF_HD float pf_feat_sample(const PfTaps2& t, const float* f1, const float* f2l, int C, float scale) {
    int e[4];
    pf_taps2_corners(t, e);
    float v[4];
    for (int j = 0; j < 4; ++j) v[j] = e[j] < 0 ? 0.f : pf_feat_dot(f1, f2l + (long)e[j] * C, C) * scale;
    float acc = v[0] * t.w[0];
    acc = acc + v[1] * t.w[1];
    acc = acc + v[2] * t.w[2];
    acc = acc + v[3] * t.w[3];
    return acc;
}
// The tap geometry of pf_lookup_elem: own view x wrapped mod W_i, zero padded; the cross view samples the LEVEL-0 grid at
// level-i coordinates and uses the result un-scaled at level i; raw row n correlates the OTHER branch's f1[n].
PF_HD PfTaps2 pf_lookup_feat_tap(const PfLookupFeatArgs& a, long b, long n, int lvl, int tap, bool cross) {
    const long N = (long)a.H * a.W;
    const int ta = tap / 9, tb = tap % 9;
    const int Hl = a.H >> lvl, Wl = a.W >> lvl;
    const float inv = 1.f / (float)(1 << lvl);                     // coords / 2**i : exact
    const float cx = a.coords[(b * 2 + 0) * N + n] * inv + (float)(ta - PF_CORR_RADIUS);
    const float cy = a.coords[(b * 2 + 1) * N + n] * inv + (float)(tb - PF_CORR_RADIUS);
    if (!cross) return pf_taps0v(pf_pymod(cx, (float)Wl), cy, Hl, Wl);
    const PfTaps2 tg = pf_taps0v(pf_pymod(cx, (float)a.W), cy, a.H, a.W);
    const float gx = pf_apply_v(tg, a.g_w2c), gy = pf_apply_v(tg, a.g_w2c + N);
    return pf_taps0v(pf_pymod(gx, (float)Wl), gy, Hl, Wl);
}
PF_HD void pf_lookup_feat_elem(long idx, const PfLookupFeatArgs& a) {  // idx over B*N*324
    const long N = (long)a.H * a.W;
    const int k = (int)(idx % PF_CORR_CH);
    const long row = idx / PF_CORR_CH;
    const long b = row / N, n = row % N;
    const int lvl = k / PF_TAPS;
    const long lsz = (long)(a.H >> lvl) * (a.W >> lvl);
    const PfTaps2 to = pf_lookup_feat_tap(a, b, n, lvl, k % PF_TAPS, false);
    const PfTaps2 tc = pf_lookup_feat_tap(a, b, n, lvl, k % PF_TAPS, true);
    a.own_out[row * a.ld + k] = pf_feat_sample(to, a.f1_own + row * a.C, a.f2_own[lvl] + b * lsz * a.C, a.C, a.scale);
    a.raw_out[row * a.ld + k] = pf_feat_sample(tc, a.f1_oth + row * a.C, a.f2_oth[lvl] + b * lsz * a.C, a.C, a.scale);
}

// K4(c): rotate the raw cross-view lookup back and add the own-view lookup
// (core/corr.py:138; core/prior_raft.py:187-188).
struct PfCombineArgs {
    const float* own; const float* raw;   // channel-last [B*N][ld]
    const float* g_back;                  // [2,N]
    float* out;                           // channel-last [B*N][ld_out]
    int B, H, W, ld, ld_out;
};
PF_HD void pf_combine_elem(long idx, const PfCombineArgs& a) {  // idx over B*N*324
    const long N = (long)a.H * a.W;
    const int k = (int)(idx % PF_CORR_CH);
    const long row = idx / PF_CORR_CH;
    const long b = row / N, n = row % N;
    const PfTaps t = pf_taps0(pf_pymod(a.g_back[n], (float)a.W), a.g_back[N + n], a.H, a.W);
    const float cross = pf_apply_ld(t, a.raw + b * N * a.ld + k, a.ld);
    a.out[row * a.ld_out + k] = a.own[row * a.ld + k] + cross;
}

// ----------------------------------------------------------------------------------------------
// Backward of K3 + K4 (SURVEY.md 8f-3 groundwork).  coords are detached every iteration
// (core/prior_raft.py:171,176) and the sample grids are constants, so the only gradients are those of the
// sampled VALUES: the bilinear weights of the forward, scattered.
//   combine:  corr = own + rotate_back(raw)  =>  d_own = d_corr (no kernel), d_raw[idx_k(p)] += w_k(p) d_corr[p]
//   lookup:   own[n][k] = sum_j w_j pyr_own[lvl][n][idx_j]   =>  g_own[lvl][n][idx_j]   += w_j d_own[n][k]
//             raw[n][k] = sum_j w_j pyr_oth[lvl][n][idx_j'] =>  g_other[lvl][n][idx_j'] += w_j d_raw[n][k]
// Gradients are ACCUMULATED (fp32 atomics; callers zero the buffers once per step).
// ----------------------------------------------------------------------------------------------
struct PfCombineBwdArgs {
    const float* d_corr;                  // channel-last [B*N][ld_in]
    const float* g_back;                  // [2,N]
    float* d_raw;                         // channel-last [B*N][ld]  (accumulated)
    int B, H, W, ld_in, ld;
};
PF_HD void pf_combine_bwd_elem(long idx, const PfCombineBwdArgs& a) {   // idx over B*N*324
    const long N = (long)a.H * a.W;
    const int k = (int)(idx % PF_CORR_CH);
    const long row = idx / PF_CORR_CH;
    const long b = row / N, n = row % N;
    const PfTaps t = pf_taps0(pf_pymod(a.g_back[n], (float)a.W), a.g_back[N + n], a.H, a.W);
    const float g = a.d_corr[row * a.ld_in + k];
    float* base = a.d_raw + b * N * a.ld + k;
    for (int j = 0; j < 4; ++j)
        if (t.w[j] != 0.f) PF_ATOMIC_ADD(base + (long)t.idx[j] * a.ld, g * t.w[j]);
}
// ----------------------------------------------------------------------------------------------
// SepConvGRU gate backward (core/update.py:46-60; one half-step):
//   z = sigmoid(az), r = sigmoid(ar), q = tanh(aq(cat[r*h, x])), h' = (1 - z) * h + z * q
// stage Q  (before the dgrad of convq):  dq_pre = dh' * z * (1 - q^2),  dz = dh' * q - dh' * h,  dh = dh' * (1 - z)
// stage ZR (after it, d_rh = gradient of r*h): dz_pre = dz * (1 - z) * z,  dr_pre = (d_rh * h) * (1 - r) * r,
//                                              dh += d_rh * r
// (the products are written in the order of torch's sigmoid_backward / tanh_backward / mul backward).
// dzr_pre is the [z | r] gradient of the fused z|r convolution (columns 0..C-1 and C..2C-1).
// ----------------------------------------------------------------------------------------------
struct PfGruQBwdArgs {
    const float* dhn; const float* z; const float* q; const float* h;
    float* dq_pre; float* dz; float* dh;
    int ld_dhn, ld_z, ld_q, ld_h, ld_dq, ld_dz, ld_dh, C;
};
PF_HD void pf_gru_q_bwd_elem(long idx, const PfGruQBwdArgs& a) {          // idx over rows*C
    const long row = idx / a.C; const int c = (int)(idx % a.C);
    const float g = a.dhn[row * a.ld_dhn + c], z = a.z[row * a.ld_z + c], q = a.q[row * a.ld_q + c], h = a.h[row * a.ld_h + c];
    a.dq_pre[row * a.ld_dq + c] = (g * z) * (1.f - q * q);
    a.dz[row * a.ld_dz + c] = g * q - g * h;
    a.dh[row * a.ld_dh + c] = g * (1.f - z);
}
struct PfGruZrBwdArgs {
    const float* dz; const float* d_rh; const float* z; const float* r; const float* h;
    float* dzr_pre; float* dh;
    int ld_dz, ld_drh, ld_z, ld_r, ld_h, ld_dzr, ld_dh, C;
};
PF_HD void pf_gru_zr_bwd_elem(long idx, const PfGruZrBwdArgs& a) {        // idx over rows*C
    const long row = idx / a.C; const int c = (int)(idx % a.C);
    const float dz = a.dz[row * a.ld_dz + c], drh = a.d_rh[row * a.ld_drh + c];
    const float z = a.z[row * a.ld_z + c], r = a.r[row * a.ld_r + c], h = a.h[row * a.ld_h + c];
    a.dzr_pre[row * a.ld_dzr + c] = (dz * (1.f - z)) * z;
    a.dzr_pre[row * a.ld_dzr + a.C + c] = ((drh * h) * (1.f - r)) * r;
    a.dh[row * a.ld_dh + c] = a.dh[row * a.ld_dh + c] + drh * r;
}
// ----------------------------------------------------------------------------------------------
// Gradient of a SepConvGRU's input x = [inp (C) | out (wout) | flows] (core/update.py:155,133) after both half-steps
// (training loop node, prior-flow_amd/train_loop.py): dx = f1 + f2 (the two half-steps' data gradients, columns of wider
// scratch rows); d_inp += dx[:, :C] (inp feeds every iteration); d_out = dx[:, C:C+wout] where out > 0 else 0 (out is the
// ReLU output of the motion encoder's last convolution, stored in x itself).  One element = one (row, column < C + wout).
struct PfGruDxArgs {
    const float* f1; const float* f2; const float* x; float* d_inp; float* d_out;
    int ld_f1, ld_f2, ld_x, ld_dinp, ld_dout, C, wout;
};
PF_HD void pf_gru_dx_finish_elem(long idx, const PfGruDxArgs& a) {
    const int w = a.C + a.wout;
    const long row = idx / w; const int c = (int)(idx % w);
    const float dx = a.f1[row * a.ld_f1 + c] + a.f2[row * a.ld_f2 + c];
    if (c < a.C) a.d_inp[row * a.ld_dinp + c] = a.d_inp[row * a.ld_dinp + c] + dx;
    else a.d_out[row * a.ld_dout + (c - a.C)] = a.x[row * a.ld_x + c] > 0.f ? dx : 0.f;
}
// ----------------------------------------------------------------------------------------------
// Backward of  y = act(x * s[b,c] + t[b,c])  over channel-last rows [B*Np][C] (core/extractor.py:112-147):
// s, t are the scale / shift of pf_channel_stats (InstanceNorm: s = rstd, t = -mean * rstd) or the folded
// BatchNorm(eval) affine.  With xh = x*s + t and g = dy masked by the ReLU (xh > 0):
//   InstanceNorm:     dx = s * (g - mean_p(g) - xh * mean_p(g * xh))      (mean over the Np pixels of (b, c))
//   BatchNorm (eval): dx = s * g
// Three elementwise passes for InstanceNorm: partial sums over pixel chunks (fp64, fixed order), their
// reduction to the two means, the apply pass.
// ----------------------------------------------------------------------------------------------
struct PfNormBwdArgs {
    const float* dy; const float* x; const float* s; const float* t;
    double* part;          // [B][nblk][C][2]
    float* coef;           // [B][C][2]: mean(g), mean(g*xh)
    float* dx;
    int B, Np, C, nblk, relu, instance;
};
PF_HD void pf_norm_bwd_partial_elem(long idx, const PfNormBwdArgs& a) {     // idx over B*nblk*C
    const int c = (int)(idx % a.C);
    const long r = idx / a.C;
    const int blk = (int)(r % a.nblk); const long b = r / a.nblk;
    const int chunk = (a.Np + a.nblk - 1) / a.nblk;
    const int p0 = blk * chunk, p1 = (p0 + chunk < a.Np) ? p0 + chunk : a.Np;
    const float s = a.s[b * a.C + c], t = a.t[b * a.C + c];
    double s1 = 0.0, s2 = 0.0;
    int p = p0;
    for (; p + 4 <= p1; p += 4) {          // four pixels' loads in flight together; the sums keep their pixel order
        float xv[4], gv[4];
        for (int u = 0; u < 4; ++u) {
            const long e = (b * a.Np + p + u) * a.C + c;
            xv[u] = a.x[e]; gv[u] = a.dy[e];
        }
        for (int u = 0; u < 4; ++u) {
            const float xh = xv[u] * s + t;
            const float g = (a.relu && !(xh > 0.f)) ? 0.f : gv[u];
            s1 += (double)g; s2 += (double)g * (double)xh;
        }
    }
    for (; p < p1; ++p) {
        const long e = (b * a.Np + p) * a.C + c;
        const float xh = a.x[e] * s + t;
        const float g = (a.relu && !(xh > 0.f)) ? 0.f : a.dy[e];
        s1 += (double)g; s2 += (double)g * (double)xh;
    }
    a.part[idx * 2] = s1; a.part[idx * 2 + 1] = s2;
}
PF_HD void pf_norm_bwd_final_elem(long idx, const PfNormBwdArgs& a) {       // idx over B*C
    const int c = (int)(idx % a.C); const long b = idx / a.C;
    double s1 = 0.0, s2 = 0.0;
    for (int k = 0; k < a.nblk; ++k) {
        const double* q = a.part + ((b * a.nblk + k) * a.C + c) * 2;
        s1 += q[0]; s2 += q[1];
    }
    a.coef[idx * 2] = (float)(s1 / (double)a.Np); a.coef[idx * 2 + 1] = (float)(s2 / (double)a.Np);
}
PF_HD void pf_norm_bwd_apply_elem(long idx, const PfNormBwdArgs& a) {       // idx over B*Np*C
    const int c = (int)(idx % a.C);
    const long b = idx / ((long)a.Np * a.C);
    const float s = a.s[b * a.C + c], t = a.t[b * a.C + c];
    const float xh = a.x[idx] * s + t;
    const float g = (a.relu && !(xh > 0.f)) ? 0.f : a.dy[idx];
    if (a.instance) {
        const float m1 = a.coef[(b * a.C + c) * 2], m2 = a.coef[(b * a.C + c) * 2 + 1];
        a.dx[idx] = s * ((g - m1) - xh * m2);
    } else {
        a.dx[idx] = s * g;
    }
}
// ResidualBlock tail on the training tape (core/extractor.py:47): out = relu(x + y), and its backward dx = dy = (out > 0) ? g : 0
// (one launch each; 4 consecutive floats per call).
struct PfAddReluArgs { const float* x; const float* y; float* out; long n; };
PF_HD void pf_add_relu_elem(long idx, const PfAddReluArgs& a) {        // idx over ceil(n / 4)
    for (long i = idx * 4; i < idx * 4 + 4 && i < a.n; ++i) {
        const float v = a.x[i] + a.y[i];
        a.out[i] = v > 0.f ? v : 0.f;
    }
}
PF_HD void pf_relu_mask_elem(long idx, const PfAddReluArgs& a) {       // x = g, y = the forward output, out = masked g
    for (long i = idx * 4; i < idx * 4 + 4 && i < a.n; ++i) a.out[i] = a.y[i] > 0.f ? a.x[i] : 0.f;
}

// ----------------------------------------------------------------------------------------------
// BatchNorm2d with frozen statistics (freeze_bn, train_flow.py:107-108; the context encoder's norm, core/extractor.py:114-115),
// optionally with the ReLU behind it, on channel-last rows [rows][C]:
//   forward   out = [relu]( x*s + t ),  s = gamma * rsqrt(var + eps),  t = beta - mean * s
//   backward  g_m = relu ? (x*s + t > 0 ? g : 0) : g;   dx = s * g_m;   d gamma = sum g_m * xhat,  d beta = sum g_m,
//             xhat = (x - mean) * rsqrt(var + eps);  the sums: fp64 partials per (row block, channel), fixed order.
// ----------------------------------------------------------------------------------------------
struct PfBnArgs {
    const float* x; const float* dy; const float* gamma; const float* beta; const float* mean; const float* var;
    float* out;            // forward: out; backward: dx
    double* part;          // [nblk][C][2]
    float* dgamma; float* dbeta;
    float eps; long rows; int C, nblk, relu, accumulate;
};
PF_HD void pf_bn_fwd_elem(long idx, const PfBnArgs& a) {              // idx over rows*C
    const int c = (int)(idx % a.C);
    const float s = a.gamma[c] * (1.f / sqrtf(a.var[c] + a.eps));
    const float y = a.x[idx] * s + (a.beta[c] - a.mean[c] * s);
    a.out[idx] = (a.relu && !(y > 0.f)) ? 0.f : y;
}
PF_HD void pf_bn_bwd_partial_elem(long idx, const PfBnArgs& a) {      // idx over nblk*C
    const int c = (int)(idx % a.C);
    const long blk = idx / a.C;
    const long chunk = (a.rows + a.nblk - 1) / a.nblk;
    const long p0 = blk * chunk, p1 = (p0 + chunk < a.rows) ? p0 + chunk : a.rows;
    const float rstd = 1.f / sqrtf(a.var[c] + a.eps), mean = a.mean[c];
    const float s = a.gamma[c] * rstd, t = a.beta[c] - mean * s;
    double s1 = 0.0, s2 = 0.0;
    long p = p0;
    for (; p + 8 <= p1; p += 8) {          // eight rows' loads in flight together; the sums keep their row order
        float xv[8], gv[8];
        for (int u = 0; u < 8; ++u) { xv[u] = a.x[(p + u) * a.C + c]; gv[u] = a.dy[(p + u) * a.C + c]; }
        for (int u = 0; u < 8; ++u) {
            const float g = (a.relu && !(xv[u] * s + t > 0.f)) ? 0.f : gv[u];
            s1 += (double)g; s2 += (double)g * (double)((xv[u] - mean) * rstd);
        }
    }
    for (; p < p1; ++p) {
        const float xv = a.x[p * a.C + c];
        const float g = (a.relu && !(xv * s + t > 0.f)) ? 0.f : a.dy[p * a.C + c];
        s1 += (double)g; s2 += (double)g * (double)((xv - mean) * rstd);
    }
    a.part[idx * 2] = s1; a.part[idx * 2 + 1] = s2;
}
PF_HD void pf_bn_bwd_final_elem(long idx, const PfBnArgs& a) {        // idx over C
    double s1 = 0.0, s2 = 0.0;
    for (int k = 0; k < a.nblk; ++k) {
        const double* q = a.part + ((long)k * a.C + idx) * 2;
        s1 += q[0]; s2 += q[1];
    }
    if (a.accumulate) { a.dbeta[idx] += (float)s1; a.dgamma[idx] += (float)s2; }
    else { a.dbeta[idx] = (float)s1; a.dgamma[idx] = (float)s2; }
}
PF_HD void pf_bn_bwd_apply_elem(long idx, const PfBnArgs& a) {        // idx over rows*C
    const int c = (int)(idx % a.C);
    const float s = a.gamma[c] * (1.f / sqrtf(a.var[c] + a.eps));
    const float y = a.x[idx] * s + (a.beta[c] - a.mean[c] * s);
    a.out[idx] = (a.relu && !(y > 0.f)) ? 0.f : s * a.dy[idx];
}

struct PfLookupBwdArgs {
    const float* coords;                  // planar [B,2,N]
    const float* g_w2c;                   // [2,N]
    const float* d_own; const float* d_raw;      // channel-last [B*N][ld]
    float* g_own[PF_CORR_LEVELS];         // level i: [B*N][H_i*W_i]  (accumulated)
    float* g_other[PF_CORR_LEVELS];
    int B, H, W, ld;
    float* clear_raw;                     // NULL, or d_raw again: every value read is replaced by 0 (the next pf_dccl_combine_bwd scatters into it)
};
PF_HD void pf_lookup_bwd_elem(long idx, const PfLookupBwdArgs& a) {     // idx over B*N*324
    const long N = (long)a.H * a.W;
    const int k = (int)(idx % PF_CORR_CH);
    const long row = idx / PF_CORR_CH;
    const long b = row / N, n = row % N;
    const int lvl = k / PF_TAPS, tap = k % PF_TAPS;
    // Consecutive lanes take taps that are neighbours in X (channel = 81 lvl + 9 ta + tb with the slow axis a offsetting x,
    // core/corr.py:120-126): their four corners then fall into the same one or two 64-byte lines of a map row, and a wave's atomic
    // instruction is a few line requests instead of one per lane (channel order, tb fastest, walks down a column: every lane its
    // own line)
#ifdef PF_LKB_CHANNEL_ORDER
    const int ta = tap / 9, tb = tap % 9;
#else
    const int ta = tap % 9, tb = tap / 9;
#endif
    const int kk = lvl * PF_TAPS + ta * 9 + tb;       // the channel this thread scatters
    const int Hl = a.H >> lvl, Wl = a.W >> lvl;
    const float inv = 1.f / (float)(1 << lvl);
    const float cx = a.coords[(b * 2 + 0) * N + n] * inv + (float)(ta - PF_CORR_RADIUS);
    const float cy = a.coords[(b * 2 + 1) * N + n] * inv + (float)(tb - PF_CORR_RADIUS);
    const long lsz = (long)Hl * Wl;
    const float go = a.d_own[row * a.ld + kk], gr = a.d_raw[row * a.ld + kk];
    if (a.clear_raw) a.clear_raw[row * a.ld + kk] = 0.f;
    const PfTaps t = pf_taps0(pf_pymod(cx, (float)Wl), cy, Hl, Wl);
    float* own = a.g_own[lvl] + row * lsz;
    for (int j = 0; j < 4; ++j)
        if (t.w[j] != 0.f) PF_ATOMIC_ADD(own + t.idx[j], go * t.w[j]);
    // cross view: the level-i coordinates index the LEVEL-0 grid (core/corr.py:132-133)
    const PfTaps tg = pf_taps0(pf_pymod(cx, (float)a.W), cy, a.H, a.W);
    const float gx = pf_apply(tg, a.g_w2c), gy = pf_apply(tg, a.g_w2c + N);
    const PfTaps to = pf_taps0(pf_pymod(gx, (float)Wl), gy, Hl, Wl);
    float* oth = a.g_other[lvl] + row * lsz;
    for (int j = 0; j < 4; ++j)
        if (to.w[j] != 0.f) PF_ATOMIC_ADD(oth + to.idx[j], gr * to.w[j]);
}

// Backward of build_pyramid (core/corr.py:99-111: three F.avg_pool2d(2, stride 2), odd sizes floor): the dense
// volume gradient  dV[row][y][x] = g0 + g1[y/2][x/2]/4 + g2[y/4][x/4]/16 + g3[y/8][x/8]/64, a parent
// contributing only where it exists (y>>i < H>>i and the whole chain of windows was complete).  Written in
// place into the level-0 gradient; one pass.  (The feature gradients are then two plain GEMMs, dV f2 and dV^T f1.)
struct PfPyramidBwdArgs { float* g0; const float* g1; const float* g2; const float* g3; long rows; int H, W; };
PF_HD void pf_pyramid_bwd_elem(long idx, const PfPyramidBwdArgs& a) {    // idx over rows*H*W
    const int N = a.H * a.W;
    const long row = idx / N;
    const int n = (int)(idx % N), y = n / a.W, x = n % a.W;
    float v = a.g0[idx];
    int hy = a.H, hx = a.W, py = y, px = x;
    const float* lv[3] = {a.g1, a.g2, a.g3};
    float scale = 1.f;
    for (int i = 0; i < 3; ++i) {
        hy >>= 1; hx >>= 1; py >>= 1; px >>= 1;
        if (py >= hy || px >= hx) break;           // odd size: the last row / column has no parent (nor grand-parents)
        scale *= 0.25f;
        v = v + lv[i][row * ((long)hy * hx) + (long)py * hx + px] * scale;
    }
    a.g0[idx] = v;
}

// ----------------------------------------------------------------------------------------------
// K12: convex 8x upsampling (core/prior_raft.py:58-67); flow = coords1 - coords0
// ----------------------------------------------------------------------------------------------
struct PfUpsampleArgs {
    const float* coords1;   // planar [B,2,N]
    const float* mask;      // channel-last [B*N][ld], channel = 64k + 8i + j (already x0.25)
    float* out;             // NCHW [B,2,8H,8W]
    int B, H, W, ld;
};
PF_HD void pf_upsample_elem(long idx, const PfUpsampleArgs& a) {  // idx over B*8H*8W
    const int W8 = 8 * a.W, H8 = 8 * a.H;
    const long N = (long)a.H * a.W;
    const int X = (int)(idx % W8);
    const int Y = (int)((idx / W8) % H8);
    const long b = idx / ((long)W8 * H8);
    const int x = X >> 3, j = X & 7, y = Y >> 3, i = Y & 7;
    const float* mrow = a.mask + (b * N + (long)y * a.W + x) * a.ld + 8 * i + j;
    float lg[9];
    float mx = -INFINITY;
    for (int k = 0; k < 9; ++k) { lg[k] = mrow[64 * k]; mx = fmaxf(mx, lg[k]); }
    float den = 0.f;
    for (int k = 0; k < 9; ++k) { lg[k] = expf(lg[k] - mx); den = den + lg[k]; }
    float su = 0.f, sv = 0.f;
    for (int k = 0; k < 9; ++k) {
        const int yy = y + k / 3 - 1, xx = x + k % 3 - 1;
        float fu = 0.f, fv = 0.f;
        if (yy >= 0 && yy < a.H && xx >= 0 && xx < a.W) {      // F.unfold zero padding
            const long p = (long)yy * a.W + xx;
            fu = 8.f * (a.coords1[(b * 2 + 0) * N + p] - (float)xx);
            fv = 8.f * (a.coords1[(b * 2 + 1) * N + p] - (float)yy);
        }
        const float wk = lg[k] / den;
        su = su + wk * fu;
        sv = sv + wk * fv;
    }
    const long plane = (long)W8 * H8;
    a.out[(b * 2 + 0) * plane + (long)Y * W8 + X] = su;
    a.out[(b * 2 + 1) * plane + (long)Y * W8 + X] = sv;
}

// Backward of K12 (autograd through upsample_flow, core/prior_raft.py:58-67), one fine pixel per call:
// with w = softmax_k(mask[64k + 8i + j]) and nb_k = 8 * flow at the k-th 3x3 neighbour (zero outside),
//   d_mask[64k + 8i + j] = w_k (s_k - sum_k' w_k' s_k'),  s_k = <g, nb_k>        (written; the caller's mask is
//                                                                                  0.25 * conv: scale upstream)
//   d_flow[neighbour k]  += 8 w_k g                                              (fp32 atomics; = d coords1)
struct PfUpsampleBwdArgs {
    const float* coords1;   // planar [B,2,N]
    const float* mask;      // channel-last [B*N][ld]
    const float* g;         // NCHW [B,2,8H,8W]: gradient of the upsampled flow
    float* d_mask;          // channel-last [B*N][ld_d]  (every one of the 576 columns is written)
    float* d_flow;          // planar [B,2,N]  (accumulated)
    int B, H, W, ld, ld_d;
};
PF_HD void pf_upsample_bwd_elem(long idx, const PfUpsampleBwdArgs& a) {  // idx over B*8H*8W
    const int W8 = 8 * a.W, H8 = 8 * a.H;
    const long N = (long)a.H * a.W;
    const int X = (int)(idx % W8);
    const int Y = (int)((idx / W8) % H8);
    const long b = idx / ((long)W8 * H8);
    const int x = X >> 3, j = X & 7, y = Y >> 3, i = Y & 7;
    const long prow = b * N + (long)y * a.W + x;
    const float* mrow = a.mask + prow * a.ld + 8 * i + j;
    const long plane = (long)W8 * H8;
    const float gu = a.g[(b * 2 + 0) * plane + (long)Y * W8 + X], gv = a.g[(b * 2 + 1) * plane + (long)Y * W8 + X];
    float w[9], sk[9];
    float mx = -INFINITY;
    for (int k = 0; k < 9; ++k) { w[k] = mrow[64 * k]; mx = fmaxf(mx, w[k]); }
    float den = 0.f;
    for (int k = 0; k < 9; ++k) { w[k] = expf(w[k] - mx); den = den + w[k]; }
    float dot = 0.f;
    for (int k = 0; k < 9; ++k) {
        const int yy = y + k / 3 - 1, xx = x + k % 3 - 1;
        w[k] = w[k] / den;
        sk[k] = 0.f;
        if (yy >= 0 && yy < a.H && xx >= 0 && xx < a.W) {
            const long p = (long)yy * a.W + xx;
            const float fu = 8.f * (a.coords1[(b * 2 + 0) * N + p] - (float)xx);
            const float fv = 8.f * (a.coords1[(b * 2 + 1) * N + p] - (float)yy);
            sk[k] = gu * fu + gv * fv;
            PF_ATOMIC_ADD(a.d_flow + (b * 2 + 0) * N + p, 8.f * w[k] * gu);
            PF_ATOMIC_ADD(a.d_flow + (b * 2 + 1) * N + p, 8.f * w[k] * gv);
        }
        dot = dot + w[k] * sk[k];
    }
    float* drow = a.d_mask + prow * a.ld_d + 8 * i + j;
    for (int k = 0; k < 9; ++k) drow[64 * k] = w[k] * (sk[k] - dot);
}

// coords1 += delta  (core/prior_raft.py:193,196); delta is channel-last [B*N][ld]
struct PfCoordsAddArgs { float* coords1; const float* delta; int B, N, ld; const float* src; };   // src: coords1 = src + delta (NULL: in place)
PF_HD void pf_coords_add_elem(long idx, const PfCoordsAddArgs& a) {   // idx over B*N
    const long b = idx / a.N, n = idx % a.N;
    const float* from = a.src ? a.src : a.coords1;
    a.coords1[(b * 2 + 0) * a.N + n] = from[(b * 2 + 0) * a.N + n] + a.delta[idx * a.ld + 0];
    a.coords1[(b * 2 + 1) * a.N + n] = from[(b * 2 + 1) * a.N + n] + a.delta[idx * a.ld + 1];
}

// ----------------------------------------------------------------------------------------------
// small direct convolution, channel-last, stride 1, "same" zero padding, optional ReLU.
// Used for the tiny-Cin layers (7x7 2->128, 3x3 8->32, 3x3 32->16; core/update.py:171-178,
// :87).  Weights packed [KH*KW][Cin][Cout].
// ----------------------------------------------------------------------------------------------
struct PfDirectConvArgs {
    const float* in; int ld_in, c_in_off, Cin;
    const float* w; const float* bias;
    float* out; int ld_out, c_out_off, Cout;
    int B, H, W, KH, KW, relu;      // H, W: OUTPUT map
    int stride, nchw, Hin, Win;     // input map = stride x output; nchw: input is [B,Cin,Hin,Win] planes
    void* out_split; int lds_out;   // optional split twin of `out` (same channel offset); `out` may then be null
    int out_f16;                    // out_split is an f16 map (PF_PREC_F16 operand) instead of a split twin
};
PF_HD void pf_direct_conv_elem(long idx, const PfDirectConvArgs& a) {  // idx over B*N*Cout
    const long N = (long)a.H * a.W, Nin = (long)a.Hin * a.Win;
    const int co = (int)(idx % a.Cout);
    const long row = idx / a.Cout;
    const long b = row / N, n = row % N;
    const int y = (int)(n / a.W) * a.stride, x = (int)(n % a.W) * a.stride;
    const int ph = a.KH / 2, pw = a.KW / 2;
    float acc = 0.f;
    for (int kh = 0; kh < a.KH; ++kh) {
        const int yy = y + kh - ph;
        if (yy < 0 || yy >= a.Hin) continue;
        for (int kw = 0; kw < a.KW; ++kw) {
            const int xx = x + kw - pw;
            if (xx < 0 || xx >= a.Win) continue;
            const float* wp = a.w + ((long)(kh * a.KW + kw) * a.Cin) * a.Cout + co;
            for (int c = 0; c < a.Cin; ++c) {
                const float v = a.nchw ? a.in[(b * a.Cin + c) * Nin + (long)yy * a.Win + xx]
                                       : a.in[(b * Nin + (long)yy * a.Win + xx) * a.ld_in + a.c_in_off + c];
                acc = acc + v * wp[(long)c * a.Cout];
            }
        }
    }
    acc = acc + a.bias[co];
    if (a.relu) acc = fmaxf(acc, 0.f);
    if (a.out) a.out[row * a.ld_out + a.c_out_off + co] = acc;
    if (a.out_split) {
        if (a.out_f16) pf_f16_put(a.out_split, row, a.lds_out, a.c_out_off + co, acc);
        else pf_split_put(a.out_split, row, a.lds_out, a.c_out_off + co, acc);
    }
}

// ----------------------------------------------------------------------------------------------
// FlowHead.conv2 (3x3, C->2, core/update.py:10,13-14) fused with the coordinate update
// coords1 += delta_flow (core/prior_raft.py:193,196).  w packed [2][9][C]; x channel-last.
// Scalar statement (host/emu); the device kernel spreads C over a wavefront.
// ----------------------------------------------------------------------------------------------
struct PfFlowOutArgs {
    const float* x; int ld, C;
    const float* w; const float* bias;
    float* coords1;            // planar [B,2,N], updated in place
    float* delta;              // optional channel-last [B*N][ld_delta] copy of delta_flow
    int ld_delta;
    int B, H, W;
};
PF_HD void pf_flow_out_elem(long idx, const PfFlowOutArgs& a) {   // idx over B*N*2
    const long N = (long)a.H * a.W;
    const int o = (int)(idx & 1);
    const long row = idx >> 1;
    const long b = row / N, n = row % N;
    const int y = (int)(n / a.W), x = (int)(n % a.W);
    float acc = 0.f;
    for (int t = 0; t < 9; ++t) {
        const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
        if (yy < 0 || yy >= a.H || xx < 0 || xx >= a.W) continue;
        const float* xp = a.x + (b * N + (long)yy * a.W + xx) * a.ld;
        const float* wp = a.w + ((long)o * 9 + t) * a.C;
        for (int c = 0; c < a.C; ++c) acc = acc + xp[c] * wp[c];
    }
    acc = acc + a.bias[o];
    if (a.delta) a.delta[row * a.ld_delta + o] = acc;
    a.coords1[(b * 2 + o) * N + n] += acc;
}

// ----------------------------------------------------------------------------------------------
// fp32 -> bf16 hi|lo split rows (operand format of the PF_PREC_BF16X3 GEMMs):
// out row = [C/32 chunks] x { bf16 hi[32], bf16 lo[32] }, hi = bf16_rne(x), lo = bf16_rne(x - hi).
// ----------------------------------------------------------------------------------------------
struct PfSplitArgs { const float* in; unsigned short* out; long rows; int C; };
PF_HD void pf_split_bf16_elem(long idx, const PfSplitArgs& a) {   // idx over rows*C/4
    const int c4n = a.C / 4;
    const int c = (int)(idx % c4n) * 4;
    const long row = idx / c4n;
    unsigned short* o = a.out + row * 2 * a.C + (c / 32) * 64 + (c % 32);
    for (int i = 0; i < 4; ++i) {
        const float x = a.in[row * a.C + c + i];
        const unsigned short hi = pf_bf16_rne(x);
        o[i] = hi;
        o[32 + i] = pf_bf16_rne(x - pf_bf16_to_f32(hi));
    }
}

// fp32 rows -> f16 map (operand format of the PF_PREC_F16 update-block convolutions): out row = lds units of 64 fp16
// channels, channel c of row r at out[r * lds * 64 + c] = fp16_rne(in[r * ld_in + c]); columns >= C are not written.
struct PfSplitF16Args { const float* in; unsigned short* out; long rows; int C, ld_in, lds; };
PF_HD void pf_split_f16_elem(long idx, const PfSplitF16Args& a) {   // idx over rows*C/4
    const int c4n = a.C / 4;
    const int c = (int)(idx % c4n) * 4;
    const long row = idx / c4n;
    const float* x = a.in + row * a.ld_in + c;
    const unsigned long long v = (unsigned long long)pf_f16_rne(x[0]) | ((unsigned long long)pf_f16_rne(x[1]) << 16) |
                                 ((unsigned long long)pf_f16_rne(x[2]) << 32) | ((unsigned long long)pf_f16_rne(x[3]) << 48);
    *reinterpret_cast<unsigned long long*>(a.out + row * a.lds * 64 + c) = v;          // 4 channels, one 8-byte store
}

// ----------------------------------------------------------------------------------------------
// Weight packing on the device (round 4).  nn.Conv2d weights [Cout][Cin][KH][KW] (one tensor, or two concatenated on Cout:
// the fused z|r convolution of a SepConvGRU half, core/update.py:48-49) -> the PF_PREC_BF16X3 operand of pf_conv2d:
// [Cout_pad][KH*KW][Cin_pad/32] x {bf16 hi[32], bf16 lo[32]}, zero padded, plus the padded bias vector.
//   mode 0: the forward convolution.
//   mode 1: the DATA-GRADIENT convolution dX = conv(dY, W'), W'[c][o][ky][kx] = W[o][(c + cin_rot) % Cin][KH-1-ky][KW-1-kx]:
//           its output channels are the forward input channels (rotated by cin_rot), its input channels the forward output
//           channels; no bias.
// A training step re-packs every convolution of the model after each optimizer step; with torch ops that was ~9 small
// kernels per pack (two fills, a permute copy, two bf16 casts, a subtract, a cat ...), ~800 launches per step.
// One element = one (packed output channel, tap, packed input channel).
// ----------------------------------------------------------------------------------------------
struct PfPackWArgs {
    const float* w0; const float* w1; const float* b0; const float* b1;
    unsigned short* dst_w; float* dst_b;
    int cout0, cout1, cin, kh, kw, mode, cin_rot, cout_pad, cin_pad;
};
PF_HD void pf_pack_conv_weights_elem(long idx, const PfPackWArgs& a) {
    const int taps = a.kh * a.kw;
    const int c = (int)(idx % a.cin_pad);
    const int tap = (int)((idx / a.cin_pad) % taps);
    const int o = (int)(idx / ((long)a.cin_pad * taps));
    const int cout = a.cout0 + a.cout1;
    float v = 0.f;
    if (a.mode == 0) {
        if (o < cout && c < a.cin) {
            const float* w = o < a.cout0 ? a.w0 + (long)o * a.cin * taps : a.w1 + (long)(o - a.cout0) * a.cin * taps;
            v = w[(long)c * taps + tap];
        }
        if (a.dst_b != nullptr && c == 0 && tap == 0)
            a.dst_b[o] = o < a.cout0 ? (a.b0 ? a.b0[o] : 0.f) : (o < cout ? (a.b1 ? a.b1[o - a.cout0] : 0.f) : 0.f);
    } else {
        if (o < a.cin && c < cout) {
            const int ci = (o + a.cin_rot) % a.cin;
            const float* w = c < a.cout0 ? a.w0 + (long)c * a.cin * taps : a.w1 + (long)(c - a.cout0) * a.cin * taps;
            v = w[(long)ci * taps + (taps - 1 - tap)];           // (KH-1-ky) * KW + (KW-1-kx) = taps - 1 - tap
        }
        if (a.dst_b != nullptr && c == 0 && tap == 0) a.dst_b[o] = 0.f;
    }
    unsigned short* d = a.dst_w + ((long)(o * taps + tap) * (a.cin_pad / 32) + c / 32) * 64 + (c % 32);
    const unsigned short hi = pf_bf16_rne(v);
    d[0] = hi;
    d[32] = pf_bf16_rne(v - pf_bf16_to_f32(hi));
}

// Several pf_pack_conv_weights problems in one launch (a training step re-packs ~115 operands after every optimizer step):
// job j owns the indices [start[j], start[j+1]).
#define PF_PACK_MAX_JOBS 16
struct PfPackBatchArgs {
    PfPackWArgs job[PF_PACK_MAX_JOBS];
    long start[PF_PACK_MAX_JOBS + 1];
    int n;
};
PF_HD void pf_pack_conv_weights_batch_elem(long idx, const PfPackBatchArgs& a) {
    int j = 0;
    while (j + 1 < a.n && idx >= a.start[j + 1]) ++j;
    pf_pack_conv_weights_elem(idx - a.start[j], a.job[j]);
}

// ----------------------------------------------------------------------------------------------
// Training: packed weight / bias gradients -> the parameters' own gradient tensors, several convolutions per launch.
//   gw[o][c][tap] += scale * dw[o_off + o][tap][c]      gb[o] += scale * db[o_off + o]
// dw: pf_conv2d_wgrad's layout [Cout_pad128][taps][cin_pad]; gw: [cout][cin][KH][KW] (the .grad of an nn.Conv2d weight, a view
// of the optimiser's flat gradient buffer).  o_off selects the rows of one module inside a fused convolution (convz|convr).
// One call = one element of one job; job j owns the indices [start[j], start[j+1]): cout*cin*taps weight elements, then cout
// bias elements.
// ----------------------------------------------------------------------------------------------
#define PF_UNPACK_MAX_JOBS 16
struct PfUnpackJob {
    const float* dw; const float* db; float* gw; float* gb;
    int cout, cin, taps, cin_pad, o_off; float scale;
};
struct PfUnpackArgs {
    PfUnpackJob job[PF_UNPACK_MAX_JOBS];
    long start[PF_UNPACK_MAX_JOBS + 1];
    int n;
};
PF_HD void pf_unpack_wgrads_elem(long idx, const PfUnpackArgs& a) {
    int j = 0;
    while (j + 1 < a.n && idx >= a.start[j + 1]) ++j;
    const PfUnpackJob& q = a.job[j];
    long i = idx - a.start[j];
    const long nw = (long)q.cout * q.cin * q.taps;
    if (i < nw) {
        const int tap = (int)(i % q.taps);
        const int c = (int)((i / q.taps) % q.cin);
        const int o = (int)(i / ((long)q.taps * q.cin));
        q.gw[i] += q.scale * q.dw[((long)(q.o_off + o) * q.taps + tap) * q.cin_pad + c];
    } else if (q.gb != nullptr) {
        i -= nw;
        q.gb[i] += q.scale * q.db[q.o_off + i];
    }
}

// ----------------------------------------------------------------------------------------------
// Encoder glue (core/extractor.py:41-47, :144-150): out = relu( res' + relu(y*s + t) ) with
// res' = res (identity shortcut) | res*rs + rt (normalised 1x1/2 shortcut) | absent.
// y, res, out: channel-last [B*Np][C]; s,t,rs,rt: [B][C].  One call = 4 consecutive channels.
// ----------------------------------------------------------------------------------------------
struct PfNormActArgs {
    const float* y; const float* s; const float* t;
    const float* res; const float* rs; const float* rt;
    float* out; int B, Np, C; int res_relu;
};
PF_HD void pf_norm_act_elem(long idx, const PfNormActArgs& a) {   // idx over B*Np*C/4
    const int c4n = a.C / 4;
    const int c = (int)(idx % c4n) * 4;
    const long row = idx / c4n;
    const long b = row / a.Np;
    for (int i = 0; i < 4; ++i) {
        const long e = row * a.C + c + i, pc = b * a.C + c + i;
        float v = fmaxf(a.y[e] * a.s[pc] + a.t[pc], 0.f);
        if (a.res) {
            float r = a.res[e];
            if (a.rs) r = r * a.rs[pc] + a.rt[pc];
            if (a.res_relu) r = fmaxf(r, 0.f);
            v = fmaxf(r + v, 0.f);
        }
        a.out[e] = v;
    }
}

// ----------------------------------------------------------------------------------------------
// NCHW -> channel-last slice copy with optional activation (0 none, 1 relu, 2 tanh)
// (core/prior_raft.py:136-142: net = tanh(cnet[:, :128]), inp = relu(cnet[:, 128:]))
// ----------------------------------------------------------------------------------------------
struct PfToNhwcArgs { const float* in; float* out; int B, C_total, c_begin, C, N, ld_out, c_out_off, act; };
PF_HD float pf_act(float v, int act) {
    if (act == 1) return fmaxf(v, 0.f);
    if (act == 2) return tanhf(v);
    return v;
}
PF_HD void pf_to_nhwc_elem(long idx, const PfToNhwcArgs& a) {   // idx over B*N*C
    const int c = (int)(idx % a.C);
    const long row = idx / a.C;
    const long b = row / a.N, n = row % a.N;
    const float v = a.in[(b * a.C_total + a.c_begin + c) * (long)a.N + n];
    a.out[row * a.ld_out + a.c_out_off + c] = pf_act(v, a.act);
}

// 2x2 space-to-depth of an NCHW image into a channel-last map:
//   out[b][Y][X][(py*2+px)*C + c] = in[b][c][2Y+py][2X+px]
// The encoders' 7x7 stride-2 stem (core/extractor.py:122, Cin = 3) is, on this image, a 4x4
// stride-1 convolution over 12 channels with window rows Y-2..Y+1 (tap KY <-> ky = 2 KY + py - 1),
// which the implicit-GEMM conv kernels run directly (see engine.EncoderPlan).
struct PfS2dArgs { const float* in; float* out; int B, C, H, W, ld_out; };   // H, W: INPUT size (even)
PF_HD void pf_s2d_elem(long idx, const PfS2dArgs& a) {           // idx over B*(H/2)*(W/2)*4*C
    const int C4 = 4 * a.C, Wo = a.W / 2, Ho = a.H / 2;
    const int cc = (int)(idx % C4);
    const long pix = idx / C4;
    const int X = (int)(pix % Wo), Y = (int)((pix / Wo) % Ho);
    const long b = pix / ((long)Wo * Ho);
    const int q = cc / a.C, c = cc % a.C;
    const int py = q >> 1, px = q & 1;
    a.out[pix * a.ld_out + cc] = a.in[((b * a.C + c) * a.H + 2 * Y + py) * (long)a.W + 2 * X + px];
}

// ----------------------------------------------------------------------------------------------
// Evaluation counterpart: per-pixel EPE and SEPE of a predicted flow against the
// ground truth.  EPE = |flow - gt| (evaluate.py:265); SEPE = haversine great-circle distance on the
// unit sphere between the two END POINTS (core/utils/spherical.py:20-53, method 'Haversine'):
// end point x wraps, y clamps (core/utils/projection_prim_ortho.py:200-218), pixel -> (theta, phi)
// by ERP.plane2spherical (:397-411).
// ----------------------------------------------------------------------------------------------
struct PfFlowMetricsArgs { const float* pred; const float* gt; float* epe; float* sd; int B, H, W; int cosine; };
PF_HD void pf_endpoint_sph(float x, float y, float u, float v, int H, int W, float& theta, float& phi) {
    const float pi = 3.14159265358979323846f;
    const float e0 = pf_pymod(x + u + 0.5f, (float)W) - 0.5f;
    float e1 = y + v;
    e1 = e1 < -0.5f ? -0.5f : (e1 > (float)H - 0.5f ? (float)H - 0.5f : e1);
    theta = (((e0 + 0.5f) / (float)W - 0.5f) * 2.f) * pi;
    phi = (0.5f - (e1 + 0.5f) / (float)H) * pi;
}
PF_HD float pf_haversine(float x) { const float s = sinf(x / 2.f); return s * s; }
PF_HD void pf_flow_metrics_elem(long idx, const PfFlowMetricsArgs& a) {   // idx over B*H*W
    const long N = (long)a.H * a.W;
    const long b = idx / N, n = idx % N;
    const float x = (float)(n % a.W), y = (float)(n / a.W);
    const float pu = a.pred[(b * 2 + 0) * N + n], pv = a.pred[(b * 2 + 1) * N + n];
    const float gu = a.gt[(b * 2 + 0) * N + n], gv = a.gt[(b * 2 + 1) * N + n];
    const float du = pu - gu, dv = pv - gv;
    if (a.epe) a.epe[idx] = sqrtf(du * du + dv * dv);
    if (a.sd) {
        float tp, pp, tg, pg;
        pf_endpoint_sph(x, y, pu, pv, a.H, a.W, tp, pp);
        pf_endpoint_sph(x, y, gu, gv, a.H, a.W, tg, pg);
        if (a.cosine) {         // method='Cosine' (core/utils/spherical.py:40-46): spherical law of cosines, as written there
            // fp32 rounding takes cos(alpha) of coincident end points past 1 and the haversine of antipodal ones past 1 (a few
            // per cent of the pixels of such a map): clamped like pf_fb_dist, with comparisons so that a NaN stays a NaN
            float ca = sinf(pp) * sinf(pg) + (cosf(pp) * cosf(pg)) * cosf(tg - tp);
            ca = ca < -1.f ? -1.f : (ca > 1.f ? 1.f : ca);
            a.sd[idx] = acosf(ca);
        } else {
            float hv = pf_haversine(pg - pp) + (cosf(pp) * cosf(pg)) * pf_haversine(tg - tp);
            hv = hv < 0.f ? 0.f : (hv > 1.f ? 1.f : hv);
            a.sd[idx] = 2.f * asinf(sqrtf(hv));
        }
    }
}

// ----------------------------------------------------------------------------------------------
// Forward-backward consistency of two opposite ERP flows (include/priorflow_hip.h: pf_fb_check).
// pf_fb_pixel is the whole statement for one pixel of one direction; pf_fb_check_elem wraps it per pixel, the device's
// 4-pixels-per-thread kernel (pf_elem_kernels.hip) calls the same function, so both forms give the same bits.
// ----------------------------------------------------------------------------------------------
struct PfFbCheckArgs {
    const float* fw; const float* bw;            // [B,2,H,W]
    unsigned char* occ_fw; unsigned char* occ_bw;   // [B,H,W]
    float* res_fw; float* res_bw;                // [B,2,H,W]
    int B, H, W, metric; float alpha, beta;
};
struct PfFbOut { float ru, rv; unsigned char occ; };
PF_HD bool pf_finite(float v) { return fabsf(v) <= 3.402823466e38f; }
PF_HD float pf_fb_phi(float y, int H) { return (0.5f - (y + 0.5f) / (float)H) * 3.14159265358979323846f; }
// Haversine distance of two ERP points from the cosines of their latitudes and their PIXEL difference (dx, dy): the angle
// differences are formed from the (small) pixel differences, not from two large angles; the haversine is clamped to [0, 1]
// (past a pole the product of the cosines is negative)
PF_HD float pf_fb_dist(float cos_a, float cos_b, float dx, float dy, int H, int W) {
    const float pi = 3.14159265358979323846f;
    const float dth = (dx / (float)W) * (2.f * pi), dph = (dy / (float)H) * pi;
    float hv = pf_haversine(dph) + (cos_a * cos_b) * pf_haversine(dth);
    hv = hv < 0.f ? 0.f : (hv > 1.f ? 1.f : hv);
    return 2.f * asinf(sqrtf(hv));
}
// one pixel (x, y) of image b, direction dir (0: f = forward flow, g = backward; 1: the other way round), f = (fu, fv) there
PF_HD PfFbOut pf_fb_pixel(const PfFbCheckArgs& a, int dir, long b, int y, int x, float fu, float fv) {
    const long N = (long)a.H * a.W;
    const float Wf = (float)a.W;
    const float* g0 = (dir ? a.fw : a.bw) + b * 2 * N;
    const float* g1 = g0 + N;
    const float qy = (float)y + fv;
    const PfWrapTaps t = pf_wraptaps((float)x + fu, qy, a.H, a.W);        // indices always inside the map (NaN / huge included)
    const float a0 = g0[t.ia];
    const float gu = pf_wrapmix(t, a0, pf_unwrap_m(a0, g0[t.ib], Wf), pf_unwrap_m(a0, g0[t.ic], Wf), pf_unwrap_m(a0, g0[t.id], Wf));
    const float gv = pf_wrapmix(t, g1[t.ia], g1[t.ib], g1[t.ic], g1[t.id]);
    PfFbOut o;
    o.ru = pf_pymod((fu + gu) + Wf * 0.5f, Wf) - Wf * 0.5f;              // u_clip
    o.rv = fv + gv;
    if (!(pf_finite(fu) && pf_finite(fv) && pf_finite(gu) && pf_finite(gv) && pf_finite(o.ru) && pf_finite(o.rv))) {
        o.ru = 0.f; o.rv = 0.f; o.occ = 1;
        return o;
    }
    float lhs, rhs;
    if (a.metric == 0) {        // PF_FB_PLANE
        lhs = o.ru * o.ru + o.rv * o.rv;
        rhs = a.alpha * ((fu * fu + fv * fv) + (gu * gu + gv * gv)) + a.beta;
    } else {                    // PF_FB_SPHERE: the sides of the spherical triangle p, q = p + f, p + r  (q -> p + r moves by g^)
        const float cp = cosf(pf_fb_phi((float)y, a.H)), cq = cosf(pf_fb_phi(qy, a.H)), cr = cosf(pf_fb_phi((float)y + o.rv, a.H));
        const float sr = pf_fb_dist(cp, cr, o.ru, o.rv, a.H, a.W);
        const float sf = pf_fb_dist(cp, cq, fu, fv, a.H, a.W);
        const float sg = pf_fb_dist(cq, cr, gu, gv, a.H, a.W);
        const float px = 6.28318530717958647692f / Wf;                  // one pixel at the equator
        lhs = sr * sr;
        rhs = a.alpha * (sf * sf + sg * sg) + a.beta * (px * px);
    }
    o.occ = lhs > rhs ? 1 : 0;
    return o;
}
PF_HD void pf_fb_check_elem(long idx, const PfFbCheckArgs& a) {   // idx over 2*B*H*W: direction, image, pixel
    const long N = (long)a.H * a.W, BN = (long)a.B * N;
    const int dir = (int)(idx / BN);
    const long r = idx % BN, b = r / N, n = r % N;
    const float* f = (dir ? a.bw : a.fw) + b * 2 * N;
    const int y = (int)n / a.W;                  // H * W < 2^30 (checked by the entry point): a 32-bit division
    const PfFbOut o = pf_fb_pixel(a, dir, b, y, (int)n - y * a.W, f[n], f[N + n]);
    (dir ? a.occ_bw : a.occ_fw)[r] = o.occ;
    float* res = (dir ? a.res_bw : a.res_fw) + b * 2 * N;
    res[n] = o.ru; res[N + n] = o.rv;
}

// ----------------------------------------------------------------------------------------------
// Chained ERP flows: long-range flow and point tracks (include/priorflow_hip.h: pf_flow_compose, pf_track_points;
// DESIGN.md section 17).  pf_trk_point is the whole statement for one point and one flow; the dense element form, the
// device's 4-pixels-per-thread kernel (pf_elem_kernels.hip) and the sparse form call it, so all give the same bits.
// ----------------------------------------------------------------------------------------------
struct PfTrkOut { float gu, gv; unsigned char bits; };     // the displacement to add (0 when not finite), the NEW state bits
// g0: the u plane of one image's flow [2,H,W]; occ: that image's mask [H,W] or null; p = (px, py), px unwrapped
PF_HD PfTrkOut pf_trk_point(const float* g0, const unsigned char* occ, int H, int W, float px, float py) {
    const float Wf = (float)W;
    const float* g1 = g0 + (long)H * W;
    const PfWrapTaps t = pf_wraptaps(px, py, H, W);                       // indices always inside the map (NaN / huge included)
    const float a0 = g0[t.ia];
    PfTrkOut o;
    o.gu = pf_wrapmix(t, a0, pf_unwrap_m(a0, g0[t.ib], Wf), pf_unwrap_m(a0, g0[t.ic], Wf), pf_unwrap_m(a0, g0[t.id], Wf));
    o.gv = pf_wrapmix(t, g1[t.ia], g1[t.ib], g1[t.ic], g1[t.id]);
    o.bits = 0;
    if (occ) {
        const float m = pf_wrapmix(t, occ[t.ia] ? 1.f : 0.f, occ[t.ib] ? 1.f : 0.f, occ[t.ic] ? 1.f : 0.f, occ[t.id] ? 1.f : 0.f);
        if (m >= 0.5f) o.bits |= 1;                                       // PF_TRK_OCCLUDED (a NaN weight decides nothing)
    }
    if (py < -0.5f || py > (float)H - 0.5f) o.bits |= 2;                  // PF_TRK_POLE: flagged, still sampled on the clamped row
    if (!(pf_finite(px) && pf_finite(py) && pf_finite(o.gu) && pf_finite(o.gv))) {
        o.gu = 0.f; o.gv = 0.f; o.bits |= 4;                              // PF_TRK_NONFINITE
    }
    return o;
}
struct PfComposeJob {
    const float* f; const unsigned char* state_f;       // [B,2,H,W], [B,H,W] or null (read as 0)
    const float* g; const unsigned char* occ_g;         // [B,2,H,W], [B,H,W] or null
    float* out; unsigned char* state_out;               // [B,2,H,W] (may be f), [B,H,W] or null (may be state_f)
};
#define PF_COMPOSE_MAX 4
struct PfComposeArgs { PfComposeJob job[PF_COMPOSE_MAX]; int njobs, B, H, W; };
// job j, field by field from values loaded with constant indices: a kernel argument indexed by a run-time value (or chosen by
// address) would be copied to scratch memory
template <class T> PF_HD T pf_pick4(int j, T v0, T v1, T v2, T v3) { return j == 0 ? v0 : (j == 1 ? v1 : (j == 2 ? v2 : v3)); }
#define PF_COMPOSE_FIELD(m) pf_pick4(j, a.job[0].m, a.job[1].m, a.job[2].m, a.job[3].m)
PF_HD PfComposeJob pf_compose_pick(const PfComposeArgs& a, int j) {
    PfComposeJob q;
    q.f = PF_COMPOSE_FIELD(f); q.state_f = PF_COMPOSE_FIELD(state_f); q.g = PF_COMPOSE_FIELD(g);
    q.occ_g = PF_COMPOSE_FIELD(occ_g); q.out = PF_COMPOSE_FIELD(out); q.state_out = PF_COMPOSE_FIELD(state_out);
    return q;
}
#undef PF_COMPOSE_FIELD
struct PfComposeOut { float u, v; unsigned char state; };
// pixel (x, y) of image b of job q, f = (fu, fv) and the state byte sf there: out = f + g^(p), p = (x, y) + f
PF_HD PfComposeOut pf_compose_pixel(const PfComposeJob& q, int H, int W, long b, int y, int x, float fu, float fv, unsigned char sf) {
    const long N = (long)H * W;
    const PfTrkOut t = pf_trk_point(q.g + b * 2 * N, q.occ_g ? q.occ_g + b * N : nullptr, H, W, (float)x + fu, (float)y + fv);
    PfComposeOut o;
    o.u = fu + t.gu; o.v = fv + t.gv; o.state = (unsigned char)(sf | t.bits);
    return o;
}
PF_HD void pf_flow_compose_elem(long idx, const PfComposeArgs& a) {       // idx over njobs*B*H*W: job, image, pixel
    const long N = (long)a.H * a.W, BN = (long)a.B * N;
    const PfComposeJob q = pf_compose_pick(a, (int)(idx / BN));
    const long r = idx % BN, b = r / N, n = r % N;
    const int y = (int)n / a.W;                  // H * W < 2^30 (checked by the entry point): a 32-bit division
    const float* f = q.f + b * 2 * N;
    const PfComposeOut o = pf_compose_pixel(q, a.H, a.W, b, y, (int)n - y * a.W, f[n], f[N + n], q.state_f ? q.state_f[r] : 0);
    float* out = q.out + b * 2 * N;              // every read of this pixel is done: out may be f, state_out may be state_f
    out[n] = o.u; out[N + n] = o.v;
    if (q.state_out) q.state_out[r] = o.state;
}
PF_HD void pf_store2(float* p, float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef float pf_f2u __attribute__((ext_vector_type(2), aligned(4)));     // dword-aligned 8-byte store
    pf_f2u v; v.x = a; v.y = b;
    *reinterpret_cast<pf_f2u*>(p) = v;
#else
    p[0] = a; p[1] = b;
#endif
}
struct PfTrackArgs { float* pos; unsigned char* state; const float* flow; const unsigned char* occ; int B, N, H, W; };
PF_HD void pf_track_points_elem(long idx, const PfTrackArgs& a) {         // idx over B*N: pos <- pos + g^(pos), in place
    const long b = idx / a.N, hw = (long)a.H * a.W;
    const PfPair p = pf_load2(a.pos + 2 * idx);
    const PfTrkOut t = pf_trk_point(a.flow + b * 2 * hw, a.occ ? a.occ + b * hw : nullptr, a.H, a.W, p.a, p.b);
    pf_store2(a.pos + 2 * idx, p.a + t.gu, p.b + t.gv);
    a.state[idx] = (unsigned char)(a.state[idx] | t.bits);
}
PF_HD void pf_track_grid_elem(long idx, const PfTrackArgs& a) {           // idx over B*H*W: the pixel centres (x, y)
    const int n = (int)(idx % ((long)a.H * a.W)), y = n / a.W;
    pf_store2(a.pos + 2 * idx, (float)(n - y * a.W), (float)y);
}

// Region sums (evaluate.py:246-275): pixel n belongs to region r when bit r of bits[n] is set.
// partials[((b*nblk + k)*R + r)*3 + {0,1,2}] = sum epe, sum sd, sum sd*weight over block k's pixels.
struct PfRegionSumArgs {
    const float* epe; const float* sd; const float* weight; const unsigned char* bits;
    double* partials; int B, N, R, nblk;
};

// ----------------------------------------------------------------------------------------------
// Training-step counterpart, the parts that do not need the network's backward.
// Sequence loss of ONE prediction (train_flow.py:62-71): m = (valid >= 0.5 && |gt| < max_flow) * w[n],
// loss_i = sum m * (|du| + |dv|); its gradient seed d loss / d pred = i_weight * m * sign(pred - gt);
// and the metrics of train_flow.py:73-79 (epe and <1/<3/<5 px fractions over the valid pixels).
// sums[6] = { sum m*(|du|+|dv|), sum_valid epe, n_valid, n(epe<1), n(epe<3), n(epe<5) }
// ----------------------------------------------------------------------------------------------
struct PfSeqLossArgs {
    const float* pred; const float* gt; const float* valid; const float* w;   // [B,2,N] x2, [B,N], [N]
    float* grad;                 // [B,2,N] or null
    double* partials;            // [B][nblk][6]
    int B, N, nblk; float i_weight, max_flow;
};
constexpr int PF_SEQ_LOSS_MAX = 32;
struct PfSeqLossBatch {           // n terms sharing gt / valid / weight: term i = PfSeqLossArgs{pred[i], ..., grad[i], partials + i * B * nblk * 6, i_weight[i]}
    const float* pred[PF_SEQ_LOSS_MAX]; float* grad[PF_SEQ_LOSS_MAX]; float i_weight[PF_SEQ_LOSS_MAX];
    PfSeqLossArgs common;         // pred / grad / i_weight unused
    int n;
};
PF_HD PfSeqLossArgs pf_seq_loss_term(const PfSeqLossBatch& t, int i) {
    PfSeqLossArgs a = t.common;
    a.pred = t.pred[i]; a.grad = t.grad[i]; a.i_weight = t.i_weight[i];
    a.partials = t.common.partials + (long)i * t.common.B * t.common.nblk * 6;
    return a;
}
PF_HD void pf_seq_loss_pixel(const PfSeqLossArgs& a, long b, int n, double (&sums)[6]) {
    const long N = a.N;
    const float gu = a.gt[(b * 2 + 0) * N + n], gv = a.gt[(b * 2 + 1) * N + n];
    const float du = a.pred[(b * 2 + 0) * N + n] - gu, dv = a.pred[(b * 2 + 1) * N + n] - gv;
    const float mag = sqrtf(gu * gu + gv * gv);
    const bool ok = (a.valid[b * N + n] >= 0.5f) && (mag < a.max_flow);
    const float m = ok ? a.w[n] : 0.f;
    if (a.grad) {
        const float gs = a.i_weight * m;
        a.grad[(b * 2 + 0) * N + n] = du > 0.f ? gs : (du < 0.f ? -gs : 0.f);
        a.grad[(b * 2 + 1) * N + n] = dv > 0.f ? gs : (dv < 0.f ? -gs : 0.f);
    }
    sums[0] += (double)(m * (fabsf(du) + fabsf(dv)));
    if (ok) {
        const float e = sqrtf(du * du + dv * dv);
        sums[1] += (double)e; sums[2] += 1.0;
        sums[3] += e < 1.f ? 1.0 : 0.0; sums[4] += e < 3.f ? 1.0 : 0.0; sums[5] += e < 5.f ? 1.0 : 0.0;
    }
}

// sum of squares (gradient norm for clip_grad_norm_, train_flow.py:137): partials[k] = chunk sums
struct PfSumSqArgs { const float* x; double* partials; long n; int nblk; };

// AdamW (torch.optim.AdamW as train_flow.py:86-88 builds it; amsgrad off), one element:
//   g' = g * gscale (the clip coefficient); p *= 1 - lr*wd; m = b1 m + (1-b1) g'; v = b2 v + (1-b2) g'^2;
//   p -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps),  bc_k = 1 - beta_k^step
struct PfAdamWArgs { float* p; const float* g; float* m; float* v; long n;
                     float decay, b1, b2, eps, step_size, sqrt_bc2, gscale; };   // scalars rounded from double like torch's
PF_HD void pf_adamw_elem(long i, const PfAdamWArgs& a) {
    const float g = a.g[i] * a.gscale;
    float p = a.p[i];
    p = p * a.decay;                                                    // param.mul_(1 - lr * weight_decay)
    const float m = a.m[i] + (g - a.m[i]) * (1.f - a.b1);               // exp_avg.lerp_(grad, 1 - beta1)
    const float v = a.v[i] * a.b2 + (g * g) * (1.f - a.b2);             // exp_avg_sq.mul_(beta2).addcmul_(g, g, 1 - beta2)
    const float denom = sqrtf(v) / a.sqrt_bc2 + a.eps;
    p = p + (m / denom) * (-a.step_size);                               // addcdiv_(exp_avg, denom, value=-step_size)
    a.p[i] = p; a.m[i] = m; a.v[i] = v;
}

// The same update with its step-dependent scalars read from DEVICE memory (hyper = {decay, step_size, sqrt_bc2, gscale}): the
// launch arguments are then the same at every step, which is what a captured HIP graph of the training step needs -- the host
// (or, for the clip coefficient, a kernel of the graph) rewrites the four floats between replays.
struct PfAdamWDevArgs { float* p; const float* g; float* m; float* v; long n; float b1, b2, eps; const float* hyper; };
PF_HD void pf_adamw_dev_elem(long i, const PfAdamWDevArgs& a) {
    PfAdamWArgs b; b.p = a.p; b.g = a.g; b.m = a.m; b.v = a.v; b.n = a.n; b.b1 = a.b1; b.b2 = a.b2; b.eps = a.eps;
    b.decay = a.hyper[0]; b.step_size = a.hyper[1]; b.sqrt_bc2 = a.hyper[2]; b.gscale = a.hyper[3];
    pf_adamw_elem(i, b);
}

// channel-last -> NCHW (debug / boundary export)
struct PfToNchwArgs { const float* in; float* out; int B, C, N, ld_in, c_in_off; };
PF_HD void pf_to_nchw_elem(long idx, const PfToNchwArgs& a) {   // idx over B*C*N
    const long n = idx % a.N;
    const long bc = idx / a.N;
    const long b = bc / a.C, c = bc % a.C;
    a.out[idx] = a.in[(b * a.N + n) * a.ld_in + a.c_in_off + c];
}

// ----------------------------------------------------------------------------------------------
// K5: warp + groupwise correlation, per pixel (core/prior_raft.py:173-174, :77-83).
// One output pixel = 4 group means; the device kernel spreads the 256 channels over one
// wavefront (see pf_elem_kernels.hip); this scalar form is the host/emu statement.
// ----------------------------------------------------------------------------------------------
struct PfWarpGcorrArgs {
    const float* f1; const float* f2;   // channel-last [B*N][C]
    const float* coords;                // planar [B,2,N]: absolute coords, or a flow when add_grid
    PfDst dst;                          // 4 channels written at dst.c_off
    int B, H, W, C, add_grid;
};
PF_HD PfTaps pf_warp_taps(const PfWarpGcorrArgs& a, long b, long n) {
    const long N = (long)a.H * a.W;
    float x = a.coords[(b * 2 + 0) * N + n], y = a.coords[(b * 2 + 1) * N + n];
    if (a.add_grid) { x = (float)(n % a.W) + x; y = (float)(n / a.W) + y; }   // coords0 + flow
    return pf_taps0(pf_pymod(x, (float)a.W), y, a.H, a.W);
}
PF_HD void pf_warp_gcorr_elem(long idx, const PfWarpGcorrArgs& a) {   // idx over B*N*4
    const long N = (long)a.H * a.W;
    const int g = (int)(idx % 4);
    const long row = idx / 4;
    const long b = row / N, n = row % N;
    const PfTaps t = pf_warp_taps(a, b, n);
    const int cg = a.C / 4;
    const float* f2b = a.f2 + b * N * a.C;
    float acc = 0.f;
    for (int c = g * cg; c < (g + 1) * cg; ++c)
        acc = acc + a.f1[row * a.C + c] * pf_apply_ld(t, f2b + c, a.C);
    a.dst.ptr[row * a.dst.ld + a.dst.c_off + g] = acc / (float)cg;
}

// ----------------------------------------------------------------------------------------------
// Per-iteration motion inputs of one pixel, fused (core/prior_raft.py:171-182): the flows of both branches
// (coords1 - coords0), flo_rotate(flow_B) into view A, and the two feature warps + groupwise correlations whose
// sample points are coords1_A and coords0 + flow_B_A.  The scalar part below is the arithmetic of pf_flow_prep_elem
// and pf_flo_rotate_elem, statement for statement (the flow at a corner pixel is formed as coords1 - coords0 first,
// exactly what the separate flow_prep launch stored), so the fused launch is bit-identical to the five it replaces.
// ----------------------------------------------------------------------------------------------
struct PfMotionPrepArgs {
    const float* c1a; const float* c1b;      // planar coords1 [B,2,N] of branch A / branch B
    const float* g_w2c; const float* g_c2w;  // flo_rotate(flow_B): W2C = grid(R_A2B), C2W = grid(R_B2A)   [2,N] each
    const float* f1; const float* f2;        // channel-last features of view A [B*N][256]
    float* flow4_a;                          // [B*N][4]  flow_A | flow_B_A      (input of the 7x7 flow stems)
    float* flow2_b;                          // [B*N][2]  flow_B
    PfDst xa, xb;                            // GRU input tails: 4 columns (flow_A | flow_B_A) / 2 columns (flow_B)
    void* xa_split; int xa_lds;              // optional split twins of the GRU input buffers (same channel offsets as xa / xb)
    void* xb_split; int xb_lds;
    int f16;                                 // the two above are f16 maps (PF_PREC_F16 operands) instead of split twins
    float* conf; int conf_ld;                // [B*N][conf_ld]: columns 0..3 flaw_A, 4..7 flaw_B_A
    int B, H, W;
};
struct PfMotionFlows { float ua, va, ub, vb, uba, vba; };
// camera-frame flow of branch B at pixel p (pf_flow_c_at with flow_B = coords1_B - coords0 formed in place)
PF_HD void pf_flow_c_at_coords(const PfMotionPrepArgs& a, long b, int p, float& f0, float& f1) {
    const long N = (long)a.H * a.W;
    const float Wf = (float)a.W;
    const float px = (float)(p % a.W), py = (float)(p / a.W);
    const float fu = a.c1b[(b * 2 + 0) * N + p] - px, fv = a.c1b[(b * 2 + 1) * N + p] - py;
    float ex = (px + fu) + 0.5f;
    ex = pf_pymod(ex, Wf) - 0.5f;
    float ey = py + fv;
    ey = fminf(fmaxf(ey, -0.5f), (float)a.H - 0.5f);
    const PfWrapTaps t = pf_wraptaps(ex, ey, a.H, a.W);
    const float* g0 = a.g_w2c;
    const float* g1 = a.g_w2c + N;
    const float a0 = g0[t.ia];
    const float e0 = pf_wrapmix(t, a0, pf_unwrap_m(a0, g0[t.ib], Wf), pf_unwrap_m(a0, g0[t.ic], Wf),
                                pf_unwrap_m(a0, g0[t.id], Wf));
    const float e1 = pf_wrapmix(t, g1[t.ia], g1[t.ib], g1[t.ic], g1[t.id]);
    f0 = e0 - g0[p];
    f0 = pf_pymod(f0 + Wf * 0.5f, Wf) - Wf * 0.5f;     // u_clip
    f1 = e1 - g1[p];
}
PF_HD PfMotionFlows pf_motion_flows(long row, const PfMotionPrepArgs& a) {      // row = b*N + n
    const long N = (long)a.H * a.W;
    const long b = row / N, n = row % N;
    const float x = (float)(n % a.W), y = (float)(n / a.W);
    PfMotionFlows f;
    f.ua = a.c1a[(b * 2 + 0) * N + n] - x; f.va = a.c1a[(b * 2 + 1) * N + n] - y;
    f.ub = a.c1b[(b * 2 + 0) * N + n] - x; f.vb = a.c1b[(b * 2 + 1) * N + n] - y;
    const PfWrapTaps t = pf_wraptaps(a.g_c2w[n], a.g_c2w[N + n], a.H, a.W);
    float a0, a1, b0, b1, c0, c1, d0, d1;
    pf_flow_c_at_coords(a, b, t.ia, a0, a1);
    pf_flow_c_at_coords(a, b, t.ib, b0, b1);
    pf_flow_c_at_coords(a, b, t.ic, c0, c1);
    pf_flow_c_at_coords(a, b, t.id, d0, d1);
    f.uba = pf_wrapmix(t, a0, b0, c0, d0);
    f.vba = pf_wrapmix(t, a1, b1, c1, d1);
    return f;
}

// Backward of K5 (autograd through cycle_bilinear_sampler + groupwise_corr, core/prior_raft.py:173-174,
// :77-83; coords detached): with gs = d_flaw[group(c)] / (C/4),
//   d_f1[p][c]        += gs * warped_f2[p][c]
//   d_f2[corner_k][c] += gs * f1[p][c] * w_k          (fp32 atomics: several pixels sample the same corner)
// One call = one (pixel, channel); both outputs are ACCUMULATED.
struct PfWarpGcorrBwdArgs {
    const float* f1; const float* f2;   // channel-last [B*N][C]
    const float* coords;                // planar [B,2,N]
    const float* d_flaw; int ld_d, off_d;   // channel-last gradient of the 4 group means
    float* d_f1; float* d_f2;           // channel-last [B*N][C]
    int B, H, W, C, add_grid;
};
PF_HD void pf_warp_gcorr_bwd_elem(long idx, const PfWarpGcorrBwdArgs& a) {   // idx over B*N*C
    const long N = (long)a.H * a.W;
    const int c = (int)(idx % a.C);
    const long row = idx / a.C;
    const long b = row / N, n = row % N;
    PfWarpGcorrArgs fa; fa.coords = a.coords; fa.H = a.H; fa.W = a.W; fa.add_grid = a.add_grid;
    const PfTaps t = pf_warp_taps(fa, b, n);
    const int cg = a.C / 4;
    const float gs = a.d_flaw[row * a.ld_d + a.off_d + c / cg] / (float)cg;
    const float* f2b = a.f2 + b * N * a.C + c;
    PF_ATOMIC_ADD(a.d_f1 + row * a.C + c, gs * pf_apply_ld(t, f2b, a.C));
    const float v = gs * a.f1[row * a.C + c];
    float* d2 = a.d_f2 + b * N * a.C + c;
    for (int j = 0; j < 4; ++j)
        if (t.w[j] != 0.f) PF_ATOMIC_ADD(d2 + (long)t.idx[j] * a.C, v * t.w[j]);
}


// ----------------------------------------------------------------------------------------------
// forward_interpolate (core/utils/utils.py:30-58, RAFT's warm start of a sequence): every pixel (x0, y0) of a flow field moves to
// (x1, y1) = (x0 + u, y0 + v); a moved point is valid iff 0 < x1 < w and 0 < y1 < h (wrap: x1 taken modulo w, only the y test);
// every grid pixel takes the (u, v) of the valid point nearest to it (griddata 'nearest'; wrap: x distances wrap).  Positions and
// distances are float64 as in the reference (int grid + float32 flow in numpy); equally near points: the lowest source index.
// Exact search in four passes over a counting sort of the valid points into the unit cells of the grid:
//   pf_fi_zero    cell counts = 0                                cell: [B][h*w + 1] (counts, then exclusive offsets + total)
//   pf_fi_count   rank of a valid point in its cell (atomic)     rank: [B][h*w] (-1: invalid)
//   (scan)        counts -> exclusive offsets per image          (PF_FI_SCAN_LAUNCH: one workgroup per image)
//   pf_fi_scatter sorted[offset(cell) + rank] = source pixel     sorted: [B][h*w]
//   pf_fi_search  rings of cells around each target pixel, until no cell left can hold a nearer point
// ----------------------------------------------------------------------------------------------
#if defined(__HIP_DEVICE_COMPILE__)
#define PF_ATOMIC_INC_I32(ptr) atomicAdd((ptr), 1)
#else
#define PF_ATOMIC_INC_I32(ptr) __atomic_fetch_add((ptr), 1, __ATOMIC_RELAXED)
#endif
struct PfFwdInterpArgs { const float* flow; float* out; int* cell; int* rank; int* sorted; int B, h, w, wrap; };

// moved position of source pixel s of image b (float64; numpy's int + float32 -> float64), false when it is not a valid point
PF_HD bool pf_fi_moved(const PfFwdInterpArgs& a, int b, int s, double& x1, double& y1) {
    const long hw = (long)a.h * a.w;
    const float* f = a.flow + (long)b * 2 * hw;
    x1 = (double)(s % a.w) + (double)f[s];
    y1 = (double)(s / a.w) + (double)f[hw + s];
    if (!(y1 > 0.0 && y1 < (double)a.h)) return false;                 // (NaN: invalid)
    if (!a.wrap) return x1 > 0.0 && x1 < (double)a.w;
    if (!(x1 - x1 == 0.0)) return false;                                // +-inf / NaN have no position modulo w
    double m = fmod(x1, (double)a.w);                                  // numpy's float remainder: the sign of w
    if (m < 0.0) m += (double)a.w;                                     // (may round to w itself, which is 0 modulo w)
    x1 = m;
    return true;
}
PF_HD int pf_fi_cell(const PfFwdInterpArgs& a, double x1, double y1) {
    int cx = (int)floor(x1);
    if (cx >= a.w) cx -= a.w;                                           // wrap: x1 == w lies in cell 0
    return (int)floor(y1) * a.w + cx;
}

PF_HD void pf_fi_zero_elem(long idx, const PfFwdInterpArgs& a) { a.cell[idx] = 0; }   // idx over B*(h*w + 1)

PF_HD void pf_fi_count_elem(long idx, const PfFwdInterpArgs& a) {      // idx over B*h*w: one source pixel
    const long hw = (long)a.h * a.w;
    const int b = (int)(idx / hw), s = (int)(idx % hw);
    double x1, y1;
    a.rank[idx] = pf_fi_moved(a, b, s, x1, y1) ? PF_ATOMIC_INC_I32(a.cell + b * (hw + 1) + pf_fi_cell(a, x1, y1)) : -1;
}

PF_HD void pf_fi_scatter_elem(long idx, const PfFwdInterpArgs& a) {    // idx over B*h*w: one source pixel
    const int r = a.rank[idx];
    if (r < 0) return;
    const long hw = (long)a.h * a.w;
    const int b = (int)(idx / hw), s = (int)(idx % hw);
    double x1, y1;
    pf_fi_moved(a, b, s, x1, y1);
    a.sorted[b * hw + a.cell[b * (hw + 1) + pf_fi_cell(a, x1, y1)] + r] = s;
}

// the points of cell (cy, cx) against the best so far (squared float64 distance, then the lower source index)
PF_HD void pf_fi_visit(const PfFwdInterpArgs& a, int b, int cy, int cx, int x, int y, double& best, int& best_s) {
    const long hw = (long)a.h * a.w;
    const int* off = a.cell + b * (hw + 1);
    const int* srt = a.sorted + b * hw;
    const int c = cy * a.w + cx;
    for (int k = off[c]; k < off[c + 1]; ++k) {
        const int s = srt[k];
        double x1, y1;
        pf_fi_moved(a, b, s, x1, y1);
        double dx = fabs(x1 - (double)x);
        if (a.wrap) dx = fmin(dx, (double)a.w - dx);
        const double dy = y1 - (double)y;
        const double d2 = dx * dx + dy * dy;
        if (d2 < best || (d2 == best && s < best_s)) { best = d2; best_s = s; }
    }
}

// One target pixel.  Ring r holds the cells at Chebyshev distance r in cell units (x: cyclic when wrapping) from the target's own
// cell; every point of a cell outside rings 0..r lies MORE than r pixels away, so the search stops after ring r once the best
// squared distance is <= r^2 (a point of a later ring can be neither nearer nor as near).
PF_HD void pf_fi_search_elem(long idx, const PfFwdInterpArgs& a) {     // idx over B*h*w
    const long hw = (long)a.h * a.w;
    const int b = (int)(idx / hw), p = (int)(idx % hw);
    const int y = p / a.w, x = p % a.w, w = a.w;
    float* o = a.out + (long)b * 2 * hw;
    const float* f = a.flow + (long)b * 2 * hw;
    double best = 0.0;
    int best_s = -1;
    if (a.cell[b * (hw + 1) + hw] > 0) {                                // no valid point: zeros (scipy would raise)
        best = 1e300;
        const int rx = a.wrap ? w / 2 : (x > w - 1 - x ? x : w - 1 - x);
        const int ry = y > a.h - 1 - y ? y : a.h - 1 - y;
        const int rmax = rx > ry ? rx : ry;
        for (int r = 0; r <= rmax; ++r) {
            const int y0 = y - r < 0 ? 0 : y - r, y1 = y + r > a.h - 1 ? a.h - 1 : y + r;
            for (int cy = y0; cy <= y1; ++cy) {
                if (cy == y - r || cy == y + r) {                       // a top / bottom row of the ring: columns within r
                    int lo = x - r, hi = x + r;
                    if (a.wrap && 2 * r + 1 >= w) { lo = 0; hi = w - 1; }
                    if (!a.wrap) { lo = lo < 0 ? 0 : lo; hi = hi > w - 1 ? w - 1 : hi; }
                    for (int c = lo; c <= hi; ++c) pf_fi_visit(a, b, cy, a.wrap ? (c % w + w) % w : c, x, y, best, best_s);
                } else if (r > 0) {                                     // a side of the ring: the columns exactly r away
                    if (a.wrap) {
                        if (2 * r <= w) pf_fi_visit(a, b, cy, ((x - r) % w + w) % w, x, y, best, best_s);
                        if (2 * r < w) pf_fi_visit(a, b, cy, (x + r) % w, x, y, best, best_s);
                    } else {
                        if (x - r >= 0) pf_fi_visit(a, b, cy, x - r, x, y, best, best_s);
                        if (x + r < w) pf_fi_visit(a, b, cy, x + r, x, y, best, best_s);
                    }
                }
            }
            if (best_s >= 0 && best <= (double)r * (double)r) break;
        }
    }
    o[p] = best_s >= 0 ? f[best_s] : 0.f;
    o[hw + p] = best_s >= 0 ? f[hw + best_s] : 0.f;
}

// counts -> exclusive offsets of one image (and the total at [h*w]); the host statement of the device scan
PF_HD void pf_fi_scan_image(const PfFwdInterpArgs& a, int b) {
    const long hw = (long)a.h * a.w;
    int* c = a.cell + b * (hw + 1);
    int s = 0;
    for (long i = 0; i < hw; ++i) { const int v = c[i]; c[i] = s; s += v; }
    c[hw] = s;
}

// ----------------------------------------------------------------------------------------------
// Order statistic of a non-negative map (include/priorflow_hip.h: pf_order_stat): out[b] = np.sort(x[b])[k],
// bit for bit, by a radix select over the bit pattern in three passes of 11 + 11 + 10 bits.  Only integer counts are summed, so
// the result does not depend on the order of the adds.  Key of a value: its bit pattern; NaN -> 0xFFFFFFFF (ranks last, alone in
// bin 2047 of the first pass: finite values and +inf have a clear sign bit, so they end at bin 1020); a set sign bit -> 0.
//   hist:  [B][2048 + 2048 + 1024] counts of the three passes (zeroed by the first launch)
//   state: [B][2][2] (prefix, remaining rank) chosen from passes 0 and 1
// Pass p > 0 first picks the bin of pass p - 1 that holds the rank (pf_os_select_image; on the device every workgroup repeats
// that scan, pf_elem_kernels.hip), then counts the digit of the elements whose higher bits equal the prefix.
// ----------------------------------------------------------------------------------------------
#define PF_OS_HIST 5120
#if defined(__HIP_DEVICE_COMPILE__)
#define PF_ATOMIC_INC_U32(ptr) atomicAdd((ptr), 1u)
#else
#define PF_ATOMIC_INC_U32(ptr) __atomic_fetch_add((ptr), 1u, __ATOMIC_RELAXED)
#endif
struct PfOrderStatArgs { const float* x; unsigned* hist; unsigned* state; float* out; long n, k; int B, pass; };
PF_HD unsigned pf_os_key(float v) {
    union { float f; unsigned u; } c; c.f = v;
    if ((c.u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
    return (c.u >> 31) ? 0u : c.u;
}
PF_HD int pf_os_nbins(int pass) { return pass == 2 ? 1024 : 2048; }
PF_HD int pf_os_hoff(int pass) { return pass * 2048; }
PF_HD unsigned pf_os_digit(unsigned key, int pass) { return pass == 0 ? key >> 21 : (pass == 1 ? (key >> 10) & 0x7ffu : key & 0x3ffu); }
PF_HD bool pf_os_match(unsigned key, int pass, unsigned prefix) {
    return pass == 0 ? true : (pass == 1 ? (key >> 21) == prefix : (key >> 10) == prefix);
}
// rank looked for in the counts of pass 0: k, or the last value that is not NaN when k falls on a NaN
PF_HD unsigned pf_os_rank0(long n, long k, unsigned n_nan) {
    const long nn = n - (long)n_nan;
    return (unsigned)(nn <= 0 ? 0 : (k < nn ? k : nn - 1));
}
PF_HD unsigned pf_os_prefix(unsigned prefix, unsigned bin, int p) { return p == 1 ? bin : ((prefix << (p == 2 ? 11 : 10)) | bin); }
PF_HD float pf_os_value(unsigned key) { union { float f; unsigned u; } c; c.u = key; return c.f; }
// the choice made after pass p - 1 (p = 1, 2: into state; p = 3: the result), one image; the host statement of the device's scan.
// The first bin whose running count exceeds the rank; no such bin (an image of NaNs only) -> bin 0, which later passes find empty.
PF_HD void pf_os_select_image(const PfOrderStatArgs& a, int b, int p) {
    const unsigned* h = a.hist + (long)b * PF_OS_HIST + pf_os_hoff(p - 1);
    const int nb = p == 1 ? 2047 : pf_os_nbins(p - 1);                   // pass 0: the NaN bin is left out
    const unsigned prefix = p == 1 ? 0u : a.state[b * 4 + (p - 2) * 2];
    const unsigned rank = p == 1 ? pf_os_rank0(a.n, a.k, h[2047]) : a.state[b * 4 + (p - 2) * 2 + 1];
    unsigned cum = 0, bin = 0, rest = 0;
    for (int j = 0; j < nb; ++j) {
        if (cum + h[j] > rank) { bin = (unsigned)j; rest = rank - cum; break; }
        cum += h[j];
    }
    const unsigned np = pf_os_prefix(prefix, bin, p);
    if (p < 3) { a.state[b * 4 + (p - 1) * 2] = np; a.state[b * 4 + (p - 1) * 2 + 1] = rest; }
    else a.out[b] = pf_os_value(np);
}
PF_HD void pf_os_zero_elem(long idx, const PfOrderStatArgs& a) { a.hist[idx] = 0u; }      // idx over B*(PF_OS_HIST + 4): hist, then state
PF_HD void pf_os_hist_elem(long idx, const PfOrderStatArgs& a) {                           // idx over B*n (host statement of a pass)
    const long b = idx / a.n;
    const unsigned key = pf_os_key(a.x[idx]);
    const unsigned prefix = a.pass ? a.state[b * 4 + (a.pass - 1) * 2] : 0u;
    if (pf_os_match(key, a.pass, prefix)) PF_ATOMIC_INC_U32(a.hist + b * PF_OS_HIST + pf_os_hoff(a.pass) + pf_os_digit(key, a.pass));
}

// ----------------------------------------------------------------------------------------------
// Colour coding of a flow field (include/priorflow_hip.h: pf_flow_render; core/utils/flow_viz.py:28-215).
//   PF_RENDER_OMNI  (omniflow_to_image): len = great-circle length of the flow (calculate_veclen_spherical, core/utils/spherical.py:
//                   56-70: pf_flow_metrics' haversine distance from the pixel to its end point), clip = the percentile of len
//   PF_RENDER_PLANE (flow_to_image):     len = |flow|, clip = its maximum
// rad = min(len, clip) / (clip + 1e-5); a = atan2(-v, -u) / pi picks and blends two entries of the 55-entry Middlebury wheel;
// col = 1 - rad (1 - blend) (rad > 1: 0.75 blend, which the epsilon keeps unreachable); byte = floor(255 col).  All fp32.
// A pixel whose flow is not finite has len = NaN (it ranks last in the percentile) and is written as (0, 0, 0).
// ----------------------------------------------------------------------------------------------
struct PfRenderArgs { const float* flow; float* len; const float* clip; unsigned char* out; int B, H, W, mode, planar, bgr; };
struct PfRgb { unsigned char c[3]; };
PF_HD unsigned char pf_wheel(int k, int i) {          // make_colorwheel (flow_viz.py:28-75): RY 15, YG 6, GC 4, CB 11, BM 13, MR 6
    static const unsigned char wheel[55 * 3] = {
        255,0,0,  255,17,0,  255,34,0,  255,51,0,  255,68,0,
        255,85,0,  255,102,0,  255,119,0,  255,136,0,  255,153,0,
        255,170,0,  255,187,0,  255,204,0,  255,221,0,  255,238,0,
        255,255,0,  213,255,0,  170,255,0,  128,255,0,  85,255,0,
        43,255,0,  0,255,0,  0,255,63,  0,255,127,  0,255,191,
        0,255,255,  0,232,255,  0,209,255,  0,186,255,  0,163,255,
        0,140,255,  0,116,255,  0,93,255,  0,70,255,  0,47,255,
        0,24,255,  0,0,255,  19,0,255,  39,0,255,  58,0,255,
        78,0,255,  98,0,255,  117,0,255,  137,0,255,  156,0,255,
        176,0,255,  196,0,255,  215,0,255,  235,0,255,  255,0,255,
        255,0,213,  255,0,170,  255,0,128,  255,0,85,  255,0,43,
    };
    return wheel[k * 3 + i];
}
PF_HD float pf_render_len(const PfRenderArgs& a, int y, int x, float u, float v) {
    if (!(pf_finite(u) && pf_finite(v))) return pf_os_value(0x7fc00000u);
    if (a.mode == 1) return sqrtf(u * u + v * v);
    float ts, ps, te, pe;
    pf_endpoint_sph((float)x, (float)y, 0.f, 0.f, a.H, a.W, ts, ps);
    pf_endpoint_sph((float)x, (float)y, u, v, a.H, a.W, te, pe);
    float hv = pf_haversine(pe - ps) + (cosf(ps) * cosf(pe)) * pf_haversine(te - ts);
    hv = hv > 1.f ? 1.f : hv;               // an antipodal end point: sin^2 + cos^2 may round past 1, and asinf would give NaN for a finite flow
    return 2.f * asinf(sqrtf(hv));
}
PF_HD PfRgb pf_render_pixel(float len, float u, float v, float clip) {
    PfRgb o; o.c[0] = 0; o.c[1] = 0; o.c[2] = 0;
    if (!(pf_finite(u) && pf_finite(v))) return o;
    const float rad = (len < clip ? len : clip) / (clip + 1e-5f);
    const float ang = atan2f(-v, -u) / 3.14159265358979323846f;
    const float fk = (ang + 1.f) / 2.f * 54.f;
    const float kf = floorf(fk);
    int k0 = kf >= 0.f ? (kf <= 54.f ? (int)kf : 54) : 0;
    const int k1 = k0 + 1 == 55 ? 0 : k0 + 1;
    const float f = fk - kf;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < 3; ++i) {
        const float c0 = (float)pf_wheel(k0, i) / 255.f, c1 = (float)pf_wheel(k1, i) / 255.f;
        float col = (1.f - f) * c0 + f * c1;
        col = rad <= 1.f ? 1.f - rad * (1.f - col) : col * 0.75f;
        const float q = floorf(255.f * col);
        o.c[i] = (unsigned char)(q >= 0.f ? (q <= 255.f ? (int)q : 255) : 0);
    }
    return o;
}
PF_HD void pf_render_len_elem(long idx, const PfRenderArgs& a) {        // idx over B*H*W
    const long N = (long)a.H * a.W, b = idx / N;
    const int n = (int)(idx % N), y = n / a.W;
    a.len[idx] = pf_render_len(a, y, n - y * a.W, a.flow[b * 2 * N + n], a.flow[(b * 2 + 1) * N + n]);
}
PF_HD void pf_render_put(const PfRenderArgs& a, long b, long n, const PfRgb& c) {
    const long N = (long)a.H * a.W;
    for (int i = 0; i < 3; ++i) {
        const int ch = a.bgr ? 2 - i : i;
        if (a.planar) a.out[(b * 3 + ch) * N + n] = c.c[i];
        else a.out[(b * N + n) * 3 + ch] = c.c[i];
    }
}
PF_HD void pf_render_color_elem(long idx, const PfRenderArgs& a) {      // idx over B*H*W
    const long N = (long)a.H * a.W, b = idx / N, n = idx % N;
    pf_render_put(a, b, n, pf_render_pixel(a.len[idx], a.flow[b * 2 * N + n], a.flow[(b * 2 + 1) * N + n], a.clip[b]));
}

// ----------------------------------------------------------------------------------------------
// my_cycle_warp (core/utils/my_cycle_sample.py:100-115): out[b,c,y,x] = x sampled at (x + u, y + v) with cycle_grid_sample's taps
// (x wraps, y clamps; is_grid = False), the taps of a pixel shared by its C channels; optionally the photometric residual
// err[b,y,x] = mean over c of |ref - out| of the same launch.
// ----------------------------------------------------------------------------------------------
struct PfCycleWarpArgs { const float* x; const float* flo; const float* ref; float* out; float* err; int B, C, H, W; };
PF_HD void pf_cycle_warp_elem(long idx, const PfCycleWarpArgs& a) {      // idx over B*H*W
    const long N = (long)a.H * a.W, b = idx / N;
    const int n = (int)(idx % N), y = n / a.W, x = n - y * a.W;
    const PfWrapTaps t = pf_wraptaps((float)x + a.flo[b * 2 * N + n], (float)y + a.flo[(b * 2 + 1) * N + n], a.H, a.W);
    float acc = 0.f;
    for (int c = 0; c < a.C; ++c) {
        const float* s = a.x + (b * a.C + c) * N;
        const float w = pf_wrapmix(t, s[t.ia], s[t.ib], s[t.ic], s[t.id]);
        a.out[(b * a.C + c) * N + n] = w;
        if (a.err) acc = acc + fabsf(a.ref[(b * a.C + c) * N + n] - w);
    }
    if (a.err) a.err[idx] = acc / (float)a.C;
}

// Mean of x over the pixels with mask == 0 (mask NULL: all), per image: partials[(b*nblk + k)*2 + {0,1}] = fp64 sum and count of
// pixel chunk k, then out[b] = sum / count in chunk order (0 when nothing is counted).  Deterministic: no atomics.
#define PF_MM_BLOCKS 64
struct PfMaskedMeanArgs { const float* x; const unsigned char* mask; double* partials; float* out; int B, N, nblk; };
PF_HD void pf_masked_mean_final_elem(long b, const PfMaskedMeanArgs& a) {   // idx over B
    double s = 0.0, c = 0.0;
    for (int k = 0; k < a.nblk; ++k) { s += a.partials[(b * a.nblk + k) * 2]; c += a.partials[(b * a.nblk + k) * 2 + 1]; }
    a.out[b] = c > 0.0 ? (float)(s / c) : 0.f;
}
