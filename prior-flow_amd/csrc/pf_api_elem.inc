// C-ABI entry points of the per-element kernels: argument validation + args-struct filling.
// Included by pf_elem_kernels.hip (device build: PF_LAUNCH enqueues a __global__ kernel) and
// by tests/emu/pf_emu.cpp (host build: PF_LAUNCH loops on the CPU).  See
// include/priorflow_hip.h for the contract of each function.

#include "../../include/priorflow_hip.h"      // pf_direct_desc; also checks every definition below against its declaration

#define PF_REQUIRE(cond) do { if (!(cond)) return PF_ERR_BAD_ARG; } while (0)
#define PF_REQUIRE_SHAPE(cond) do { if (!(cond)) return PF_ERR_BAD_SHAPE; } while (0)

static inline PfDst pf_dst(float* p, int ld, int off) { PfDst d; d.ptr = p; d.ld = ld; d.c_off = off; return d; }

extern "C" int pf_sample_grid(float* grid, int H, int W, const float* R_host, void* stream) {
    PF_REQUIRE(grid && R_host);
    PF_REQUIRE_SHAPE(H > 1 && W > 1);
    PfGridArgs a; a.grid = grid; a.H = H; a.W = W;
    for (int i = 0; i < 9; ++i) a.R[i] = R_host[i];
    return PF_LAUNCH(sample_grid, a, (long)H * W, stream);
}

extern "C" int pf_img_rotate(const float* img, const float* grid, float* out, int B, int C, int H,
                             int W, void* stream) {
    PF_REQUIRE(img && grid && out && img != out);
    PF_REQUIRE_SHAPE(B > 0 && C > 0 && H > 1 && W > 1);
    PfImgRotArgs a; a.img = img; a.grid = grid; a.out = out; a.B = B; a.C = C; a.H = H; a.W = W;
    return PF_LAUNCH(img_rotate, a, (long)B * C * H * W, stream);
}

extern "C" int pf_normalise_images(const float* image1, const float* image2, float* f1, float* f2, float* c1,
                                   long count, void* stream) {
    PF_REQUIRE(image1 && image2 && f1 && f2 && f1 != image1 && f2 != image2 && f1 != f2);
    PF_REQUIRE_SHAPE(count > 0);
    PfNormImgArgs a; a.image1 = image1; a.image2 = image2; a.f1 = f1; a.f2 = f2; a.c1 = c1;
    return PF_LAUNCH(normalise_images, a, count, stream);
}

extern "C" int pf_prepare_images(const float* image1, const float* image2, const float* grid, float* img_f, float* img_c,
                                 int B, int H, int W, void* stream) {
    PF_REQUIRE(image1 && image2 && grid && img_f && img_f != image1 && img_f != image2 && img_c != image1 && img_c != image2);
    PF_REQUIRE_SHAPE(B > 0 && H > 1 && W > 1);
    PfPrepImgArgs a; a.image1 = image1; a.image2 = image2; a.grid = grid; a.f = img_f; a.c = img_c; a.B = B; a.H = H; a.W = W;
    return PF_LAUNCH(prepare_images, a, (long)B * 3 * H * W, stream);
}

extern "C" int pf_prepare_frame(const float* image, const float* grid, float* out, int B, int H, int W, void* stream) {
    PF_REQUIRE(image && grid && out && out != image);
    PF_REQUIRE_SHAPE(B > 0 && H > 1 && W > 1);
    PfPrepFrameArgs a; a.image = image; a.grid = grid; a.out = out; a.B = B; a.H = H; a.W = W;
    return PF_LAUNCH(prepare_frame, a, (long)B * 3 * H * W, stream);
}

#if !defined(PF_FI_SCAN_LAUNCH) && !defined(__HIPCC__)
// host build (tests/emu): the scan as its host statement, one image after the other (the device build defines the macro as the
// one-workgroup-per-image scan kernel of pf_elem_kernels.hip and never falls back to this)
static int pf_fi_scan_host(const PfFwdInterpArgs& a, void*) {
    for (int b = 0; b < a.B; ++b) pf_fi_scan_image(a, b);
    return PF_OK;
}
#define PF_FI_SCAN_LAUNCH(a, stream) pf_fi_scan_host(a, stream)
#endif

extern "C" int pf_forward_interpolate(const float* flow, float* out, void* scratch, long scratch_bytes, int B, int h, int w,
                                      int wrap, void* stream) {
    PF_REQUIRE(flow && out && scratch && flow != out && (wrap == 0 || wrap == 1));
    PF_REQUIRE_SHAPE(B > 0 && h > 0 && w > 0 && (long)h * w < (1L << 30));
    const long hw = (long)h * w;
    PF_REQUIRE(scratch_bytes >= 4L * B * (3 * hw + 1));
    PfFwdInterpArgs a; a.flow = flow; a.out = out; a.B = B; a.h = h; a.w = w; a.wrap = wrap;
    a.cell = (int*)scratch; a.rank = a.cell + B * (hw + 1); a.sorted = a.rank + B * hw;
    int rc = PF_LAUNCH(fi_zero, a, B * (hw + 1), stream);
    if (rc == PF_OK) rc = PF_LAUNCH(fi_count, a, B * hw, stream);
    if (rc == PF_OK) rc = PF_FI_SCAN_LAUNCH(a, stream);
    if (rc == PF_OK) rc = PF_LAUNCH(fi_scatter, a, B * hw, stream);
    if (rc == PF_OK) rc = PF_LAUNCH(fi_search, a, B * hw, stream);
    return rc;
}

extern "C" int pf_flow_prep(const float* coords1, float* flow_out, float* d0, int d0_ld, int d0_off,
                            float* d1, int d1_ld, int d1_off, int B, int H8, int W8, void* stream) {
    PF_REQUIRE(coords1);
    PF_REQUIRE_SHAPE(B > 0 && H8 > 0 && W8 > 0);
    PF_REQUIRE(!d0 || (d0_off >= 0 && d0_off + 2 <= d0_ld));
    PF_REQUIRE(!d1 || (d1_off >= 0 && d1_off + 2 <= d1_ld));
    PfFlowPrepArgs a; a.coords1 = coords1; a.flow = flow_out;
    a.d0 = pf_dst(d0, d0_ld, d0_off); a.d1 = pf_dst(d1, d1_ld, d1_off);
    a.B = B; a.H = H8; a.W = W8;
    return PF_LAUNCH(flow_prep, a, (long)B * H8 * W8, stream);
}

extern "C" int pf_flo_rotate(const float* flow, const float* g_w2c, const float* g_c2w, float* out,
                             float* d0, int d0_ld, int d0_off, float* d1, int d1_ld, int d1_off,
                             int B, int H8, int W8, void* stream) {
    PF_REQUIRE(flow && g_w2c && g_c2w && flow != out);
    PF_REQUIRE_SHAPE(B > 0 && H8 > 0 && W8 > 0);
    PF_REQUIRE(!d0 || (d0_off >= 0 && d0_off + 2 <= d0_ld));
    PF_REQUIRE(!d1 || (d1_off >= 0 && d1_off + 2 <= d1_ld));
    PfFloRotArgs a; a.flow = flow; a.g_w2c = g_w2c; a.g_c2w = g_c2w; a.out = out;
    a.d0 = pf_dst(d0, d0_ld, d0_off); a.d1 = pf_dst(d1, d1_ld, d1_off);
    a.B = B; a.H = H8; a.W = W8;
    return PF_LAUNCH(flo_rotate, a, (long)B * H8 * W8, stream);
}

extern "C" int pf_dccl_lookup_il(const float* coords, const float* own0, const float* own1,
                                 const float* own2, const float* own3, const float* oth0,
                                 const float* oth1, const float* oth2, const float* oth3,
                                 const float* g_w2c, const float* g_w2c_il, float* own_out, float* raw_out,
                                 int B, int H8, int W8, int ld, void* stream) {
    PF_REQUIRE(coords && own0 && own1 && own2 && own3 && oth0 && oth1 && oth2 && oth3);
    PF_REQUIRE(g_w2c && own_out && raw_out && own_out != raw_out);
    // level 3 must be at least 2x2 (the (size-1) normalisation divides by zero otherwise)
    PF_REQUIRE_SHAPE(B > 0 && (H8 >> 3) >= 2 && (W8 >> 3) >= 2 && ld >= PF_CORR_CH);
    PfLookupArgs a; a.coords = coords;
    a.own[0] = own0; a.own[1] = own1; a.own[2] = own2; a.own[3] = own3;
    a.other[0] = oth0; a.other[1] = oth1; a.other[2] = oth2; a.other[3] = oth3;
    a.g_w2c = g_w2c; a.g_il = g_w2c_il; a.own_out = own_out; a.raw_out = raw_out;
    a.B = B; a.H = H8; a.W = W8; a.ld = ld;
    return PF_LOOKUP_LAUNCH(a, (long)B * H8 * W8 * (PF_CORR_CH / PF_LOOKUP_TPT), stream);
}

extern "C" int pf_dccl_lookup(const float* coords, const float* own0, const float* own1,
                              const float* own2, const float* own3, const float* oth0,
                              const float* oth1, const float* oth2, const float* oth3,
                              const float* g_w2c, float* own_out, float* raw_out, int B, int H8,
                              int W8, int ld, void* stream) {
    return pf_dccl_lookup_il(coords, own0, own1, own2, own3, oth0, oth1, oth2, oth3, g_w2c, nullptr, own_out, raw_out,
                             B, H8, W8, ld, stream);
}

// alternate_corr (pf_elem.h: pf_feat_pool_elem, pf_lookup_feat_elem)
#ifndef PF_LOOKUP_FEAT_LAUNCH
#define PF_LOOKUP_FEAT_LAUNCH(a, total, stream) PF_LAUNCH(lookup_feat, a, total, stream)
#endif
static inline bool pf_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
// the pooled levels' sizes must reach a 2x2 level 3 (the (size-1) normalisation of the sampler divides by zero otherwise);
// C: the tuned kernel holds a lane's channels in registers (4 per 256)
#define PF_FEAT_SHAPE_OK(B, H8, W8, C) ((B) > 0 && ((H8) >> 3) >= 2 && ((W8) >> 3) >= 2 && (C) > 0 && (C) % 4 == 0 && (C) <= 512)

extern "C" int pf_feature_pyramid(const float* f2, float* l1, float* l2, float* l3, int B, int H8, int W8, int C,
                                  void* stream) {
    PF_REQUIRE(f2 && l1 && l2 && l3);
    PF_REQUIRE(pf_aligned16(f2) && pf_aligned16(l1) && pf_aligned16(l2) && pf_aligned16(l3));
    PF_REQUIRE_SHAPE(PF_FEAT_SHAPE_OK(B, H8, W8, C));
    const float* in[3] = {f2, l1, l2};
    float* out[3] = {l1, l2, l3};
    for (int i = 0; i < 3; ++i) {
        PfFeatPoolArgs a; a.in = in[i]; a.out = out[i]; a.B = B; a.H = H8 >> i; a.W = W8 >> i; a.C = C;
        const int rc = PF_LAUNCH(feat_pool, a, (long)B * (a.H >> 1) * (a.W >> 1) * (C / 4), stream);
        if (rc != PF_OK) return rc;
    }
    return PF_OK;
}

extern "C" int pf_dccl_lookup_feat(const float* coords, const float* f1_own, const float* f2_own0, const float* f2_own1,
                                   const float* f2_own2, const float* f2_own3, const float* f1_oth, const float* f2_oth0,
                                   const float* f2_oth1, const float* f2_oth2, const float* f2_oth3, const float* g_w2c,
                                   float* own_out, float* raw_out, int* path_counts, int B, int H8, int W8, int C, int ld,
                                   void* stream) {
    PF_REQUIRE(coords && f1_own && f2_own0 && f2_own1 && f2_own2 && f2_own3);
    PF_REQUIRE(f1_oth && f2_oth0 && f2_oth1 && f2_oth2 && f2_oth3);
    PF_REQUIRE(g_w2c && own_out && raw_out && own_out != raw_out);
    const float* fs[10] = {f1_own, f2_own0, f2_own1, f2_own2, f2_own3, f1_oth, f2_oth0, f2_oth1, f2_oth2, f2_oth3};
    for (int i = 0; i < 10; ++i) PF_REQUIRE(pf_aligned16(fs[i]));
    PF_REQUIRE_SHAPE(PF_FEAT_SHAPE_OK(B, H8, W8, C) && ld >= PF_CORR_CH);
    PfLookupFeatArgs a; a.coords = coords; a.f1_own = f1_own; a.f1_oth = f1_oth;
    a.f2_own[0] = f2_own0; a.f2_own[1] = f2_own1; a.f2_own[2] = f2_own2; a.f2_own[3] = f2_own3;
    a.f2_oth[0] = f2_oth0; a.f2_oth[1] = f2_oth1; a.f2_oth[2] = f2_oth2; a.f2_oth[3] = f2_oth3;
    a.g_w2c = g_w2c; a.own_out = own_out; a.raw_out = raw_out; a.path_counts = path_counts;
    a.B = B; a.H = H8; a.W = W8; a.C = C; a.ld = ld; a.scale = 1.f / sqrtf((float)C);
    return PF_LOOKUP_FEAT_LAUNCH(a, (long)B * H8 * W8 * PF_CORR_CH, stream);
}

extern "C" int pf_dccl_combine(const float* own, const float* raw, const float* g_back, float* out,
                               int B, int H8, int W8, int ld, int ld_out, void* stream) {
    PF_REQUIRE(own && raw && g_back && out && out != raw);
    PF_REQUIRE_SHAPE(B > 0 && H8 > 1 && W8 > 1 && ld >= PF_CORR_CH && ld_out >= PF_CORR_CH);
    PfCombineArgs a; a.own = own; a.raw = raw; a.g_back = g_back; a.out = out;
    a.B = B; a.H = H8; a.W = W8; a.ld = ld; a.ld_out = ld_out;
    return PF_COMBINE_LAUNCH(a, (long)B * H8 * W8 * PF_CORR_CH, stream);
}

extern "C" int pf_coords_add(float* coords1, const float* delta, int ld, int B, int H8, int W8,
                             void* stream) {
    PF_REQUIRE(coords1 && delta);
    PF_REQUIRE_SHAPE(B > 0 && H8 > 0 && W8 > 0 && ld >= 2);
    PfCoordsAddArgs a; a.coords1 = coords1; a.delta = delta; a.B = B; a.N = H8 * W8; a.ld = ld; a.src = nullptr;
    return PF_LAUNCH(coords_add, a, (long)B * H8 * W8, stream);
}

extern "C" int pf_coords_add_to(const float* src, const float* delta, int ld, float* dst, int B, int H8, int W8,
                                void* stream) {
    PF_REQUIRE(src && delta && dst);
    PF_REQUIRE_SHAPE(B > 0 && H8 > 0 && W8 > 0 && ld >= 2);
    PfCoordsAddArgs a; a.coords1 = dst; a.delta = delta; a.B = B; a.N = H8 * W8; a.ld = ld; a.src = src;
    return PF_LAUNCH(coords_add, a, (long)B * H8 * W8, stream);
}

extern "C" int pf_upsample_flow(const float* coords1, const float* mask, int ld, float* out, int B,
                                int H8, int W8, void* stream) {
    PF_REQUIRE(coords1 && mask && out);
    PF_REQUIRE_SHAPE(B > 0 && H8 > 0 && W8 > 0 && ld >= 576);
    PfUpsampleArgs a; a.coords1 = coords1; a.mask = mask; a.out = out;
    a.B = B; a.H = H8; a.W = W8; a.ld = ld;
    return PF_LAUNCH(upsample, a, (long)B * H8 * W8 * 64, stream);
}

static inline int pf_small_conv_fill(PfDirectConvArgs& a, const float* in, int nchw, int ld_in, int off_in,
                                     int cin, const float* weight, const float* bias, float* out, int ld_out,
                                     int off_out, int cout, int kh, int kw, int stride, int relu, int B,
                                     int Hout, int Wout) {
    PF_REQUIRE(in && weight && bias && in != out);       // (out may be null when the caller attaches a split twin)
    PF_REQUIRE_SHAPE(B > 0 && Hout > 0 && Wout > 0 && cin > 0 && cout > 0 && (kh & 1) && (kw & 1));
    PF_REQUIRE_SHAPE(stride == 1 || stride == 2);
    PF_REQUIRE(nchw || (off_in >= 0 && off_in + cin <= ld_in));
    PF_REQUIRE(off_out >= 0 && off_out + cout <= ld_out);
    a.in = in; a.ld_in = ld_in; a.c_in_off = off_in; a.Cin = cin;
    a.w = weight; a.bias = bias; a.out = out; a.ld_out = ld_out; a.c_out_off = off_out; a.Cout = cout;
    a.B = B; a.H = Hout; a.W = Wout; a.KH = kh; a.KW = kw; a.relu = relu;
    a.stride = stride; a.nchw = nchw; a.Hin = Hout * stride; a.Win = Wout * stride;
    a.out_split = nullptr; a.lds_out = 0; a.out_f16 = 0;
    return PF_OK;
}

extern "C" int pf_conv2d_direct(const float* in, int ld_in, int off_in, int cin, const float* weight,
                                const float* bias, float* out, int ld_out, int off_out, int cout,
                                int kh, int kw, int relu, int B, int H8, int W8, void* stream) {
    PfDirectConvArgs a;
    PF_REQUIRE(out);
    const int rc = pf_small_conv_fill(a, in, 0, ld_in, off_in, cin, weight, bias, out, ld_out, off_out, cout,
                                      kh, kw, 1, relu, B, H8, W8);
    if (rc != PF_OK) return rc;
    return PF_DIRECT_CONV_LAUNCH(a, (long)B * H8 * W8 * cout, stream);
}

static int pf_direct_group_impl(const pf_direct_desc* descs, int n, int cin, int cout, int kh, int kw, int relu,
                                int B, int H8, int W8, int f16, void* stream) {
    PF_REQUIRE(descs && n >= 1 && n <= 4);
    PfDirectConvArgs a[4];
    for (int i = 0; i < n; ++i) {
        const pf_direct_desc& d = descs[i];
        PF_REQUIRE(d.out || d.out_split);
        const int rc = pf_small_conv_fill(a[i], d.in, 0, d.ld_in, d.off_in, cin, d.weight, d.bias, d.out,
                                          d.out ? d.ld_out : d.off_out + cout, d.off_out, cout, kh, kw, 1, relu, B, H8, W8);
        if (rc != PF_OK) return rc;
        PF_REQUIRE_SHAPE(!d.out_split || (d.off_out % 8 == 0 && d.off_out + cout <= d.lds_out * (f16 ? 64 : 32)));
        a[i].out_split = d.out_split; a[i].lds_out = d.lds_out; a[i].out_f16 = f16;
        for (int k = 0; k < i; ++k)       // outputs of a group are written concurrently: they must not overlap
            PF_REQUIRE(!(descs[k].out == d.out && descs[k].out_split == d.out_split &&
                         descs[k].off_out < d.off_out + cout && d.off_out < descs[k].off_out + cout));
    }
    return PF_DIRECT_CONV_GROUP_LAUNCH(a, n, (long)B * H8 * W8 * cout, stream);
}

extern "C" int pf_conv2d_direct_group(const pf_direct_desc* descs, int n, int cin, int cout, int kh, int kw, int relu,
                                      int B, int H8, int W8, void* stream) {
    return pf_direct_group_impl(descs, n, cin, cout, kh, kw, relu, B, H8, W8, 0, stream);
}

extern "C" int pf_conv2d_direct_group_f16(const pf_direct_desc* descs, int n, int cin, int cout, int kh, int kw, int relu,
                                          int B, int H8, int W8, void* stream) {
    return pf_direct_group_impl(descs, n, cin, cout, kh, kw, relu, B, H8, W8, 1, stream);
}

extern "C" int pf_conv2d_small(const float* in, int nchw, int ld_in, int off_in, int cin,
                               const float* weight, const float* bias, float* out, int ld_out, int off_out,
                               int cout, int kh, int kw, int stride, int relu, int B, int Hout, int Wout,
                               void* stream) {
    PfDirectConvArgs a;
    PF_REQUIRE(out);
    const int rc = pf_small_conv_fill(a, in, nchw, ld_in, off_in, cin, weight, bias, out, ld_out, off_out,
                                      cout, kh, kw, stride, relu, B, Hout, Wout);
    if (rc != PF_OK) return rc;
    return PF_DIRECT_CONV_LAUNCH(a, (long)B * Hout * Wout * cout, stream);
}

extern "C" int pf_norm_act(const float* y, const float* s, const float* t, const float* res,
                           const float* rs, const float* rt, int res_relu, float* out, int B, int Np, int C, void* stream) {
    PF_REQUIRE(y && s && t && out);
    PF_REQUIRE((rs == nullptr) == (rt == nullptr) && (!rs || res) && (!res_relu || rs));
    PF_REQUIRE_SHAPE(B > 0 && Np > 0 && C > 0 && C % 4 == 0);
    PfNormActArgs a; a.y = y; a.s = s; a.t = t; a.res = res; a.rs = rs; a.rt = rt; a.out = out;
    a.B = B; a.Np = Np; a.C = C; a.res_relu = res_relu;
#ifdef PF_NORM_ACT_LAUNCH
    return PF_NORM_ACT_LAUNCH(a, (long)B * Np * (C / 4), stream);
#else
    return PF_LAUNCH(norm_act, a, (long)B * Np * (C / 4), stream);
#endif
}

extern "C" int pf_flow_head_out(const float* x, int ld, int C, const float* weight, const float* bias,
                                float* coords1, float* delta, int ld_delta, int B, int H8, int W8, void* stream) {
    PF_REQUIRE(x && weight && bias && coords1);
    PF_REQUIRE_SHAPE(B > 0 && H8 > 0 && W8 > 0 && C > 0 && C <= ld && (!delta || ld_delta >= 2));
    PfFlowOutArgs a; a.x = x; a.ld = ld; a.C = C; a.w = weight; a.bias = bias; a.coords1 = coords1;
    a.delta = delta; a.ld_delta = ld_delta; a.B = B; a.H = H8; a.W = W8;
    return PF_FLOW_OUT_LAUNCH(a, (long)B * H8 * W8 * 2, stream);
}

extern "C" int pf_split_bf16(const float* in, void* out, long rows, int C, void* stream) {
    PF_REQUIRE(in && out && (const void*)in != out);
    PF_REQUIRE_SHAPE(rows > 0 && C > 0 && C % 32 == 0);
    PfSplitArgs a; a.in = in; a.out = (unsigned short*)out; a.rows = rows; a.C = C;
    return PF_LAUNCH(split_bf16, a, rows * (C / 4), stream);
}

extern "C" int pf_split_f16(const float* in, int ld_in, void* out, int lds_out, long rows, int C, void* stream) {
    PF_REQUIRE(in && out && (const void*)in != out);
    PF_REQUIRE_SHAPE(rows > 0 && C > 0 && C % 4 == 0 && ld_in >= C && ld_in % 4 == 0 && lds_out * 64 >= C);
    PfSplitF16Args a; a.in = in; a.out = (unsigned short*)out; a.rows = rows; a.C = C; a.ld_in = ld_in; a.lds = lds_out;
    return PF_LAUNCH(split_f16, a, rows * (C / 4), stream);
}

static int pf_pack_job_args(const float* w0, int cout0, const float* w1, int cout1, const float* b0, const float* b1,
                            int cin, int kh, int kw, int mode, int cin_rot, void* dst_w, float* dst_b,
                            int cout_pad, int cin_pad, PfPackWArgs& a) {
    PF_REQUIRE(w0 && dst_w && cout0 > 0 && cout1 >= 0 && (cout1 == 0 || w1) && (mode == 0 || mode == 1));
    PF_REQUIRE_SHAPE(cin > 0 && kh > 0 && kw > 0 && kh <= 7 && kw <= 7 && cin_pad % 32 == 0 && cout_pad > 0);
    PF_REQUIRE_SHAPE(cin_rot >= 0 && cin_rot < cin);
    const int cout = cout0 + cout1;
    // packed (output, input) channels: forward (cout, cin); data gradient (cin, cout)
    PF_REQUIRE_SHAPE(mode == 0 ? (cout_pad >= cout && cin_pad >= cin) : (cout_pad >= cin && cin_pad >= cout));
    a.w0 = w0; a.w1 = w1; a.b0 = b0; a.b1 = b1; a.dst_w = (unsigned short*)dst_w; a.dst_b = dst_b;
    a.cout0 = cout0; a.cout1 = cout1; a.cin = cin; a.kh = kh; a.kw = kw; a.mode = mode; a.cin_rot = cin_rot;
    a.cout_pad = cout_pad; a.cin_pad = cin_pad;
    return PF_OK;
}

extern "C" int pf_pack_conv_weights(const float* w0, int cout0, const float* w1, int cout1, const float* b0, const float* b1,
                                    int cin, int kh, int kw, int mode, int cin_rot, void* dst_w, float* dst_b,
                                    int cout_pad, int cin_pad, void* stream) {
    PfPackWArgs a;
    const int rc = pf_pack_job_args(w0, cout0, w1, cout1, b0, b1, cin, kh, kw, mode, cin_rot, dst_w, dst_b, cout_pad, cin_pad, a);
    if (rc != PF_OK) return rc;
    return PF_LAUNCH(pack_conv_weights, a, (long)cout_pad * kh * kw * cin_pad, stream);
}

extern "C" int pf_pack_conv_weights_batch(const pf_pack_job* jobs, int n, void* stream) {
    PF_REQUIRE(jobs && n > 0);
    for (int base = 0; base < n; base += PF_PACK_MAX_JOBS) {
        PfPackBatchArgs a;
        a.n = n - base < PF_PACK_MAX_JOBS ? n - base : PF_PACK_MAX_JOBS;
        long total = 0;
        for (int j = 0; j < a.n; ++j) {
            const pf_pack_job& s = jobs[base + j];
            const int rc = pf_pack_job_args(s.w0, s.cout0, s.w1, s.cout1, s.b0, s.b1, s.cin, s.kh, s.kw, s.mode, s.cin_rot,
                                            s.dst_w, s.dst_b, s.cout_pad, s.cin_pad, a.job[j]);
            if (rc != PF_OK) return rc;
            a.start[j] = total;
            total += (long)s.cout_pad * s.kh * s.kw * s.cin_pad;
        }
        a.start[a.n] = total;
        const int rc = PF_LAUNCH(pack_conv_weights_batch, a, total, stream);
        if (rc != PF_OK) return rc;
    }
    return PF_OK;
}

extern "C" int pf_unpack_wgrads(const pf_unpack_job* jobs, int n, void* stream) {
    PF_REQUIRE(jobs && n > 0);
    for (int base = 0; base < n; base += PF_UNPACK_MAX_JOBS) {
        PfUnpackArgs a;
        a.n = n - base < PF_UNPACK_MAX_JOBS ? n - base : PF_UNPACK_MAX_JOBS;
        long total = 0;
        for (int j = 0; j < a.n; ++j) {
            const pf_unpack_job& s = jobs[base + j];
            PF_REQUIRE(s.dw && s.gw && (s.gb == nullptr || s.db != nullptr));
            PF_REQUIRE_SHAPE(s.cout > 0 && s.cin > 0 && s.taps > 0 && s.cin_pad >= s.cin && s.o_off >= 0);
            PfUnpackJob& q = a.job[j];
            q.dw = s.dw; q.db = s.db; q.gw = s.gw; q.gb = s.gb;
            q.cout = s.cout; q.cin = s.cin; q.taps = s.taps; q.cin_pad = s.cin_pad; q.o_off = s.o_off; q.scale = s.scale;
            a.start[j] = total;
            total += (long)s.cout * s.cin * s.taps + (s.gb ? s.cout : 0);
        }
        a.start[a.n] = total;
        const int rc = PF_LAUNCH(unpack_wgrads, a, total, stream);
        if (rc != PF_OK) return rc;
    }
    return PF_OK;
}

extern "C" int pf_channel_stats(const float* y, int B, int Np, int C, float eps, float* scale, float* shift,
                                double* partials, int nblk, void* stream) {
    PF_REQUIRE(y && scale && shift && partials);
    PF_REQUIRE_SHAPE(B > 0 && Np > 0 && C > 0 && C <= 256 && C % 4 == 0 && nblk > 0 && nblk <= 1024);
    return PF_STATS_LAUNCH(y, B, Np, C, eps, scale, shift, partials, nblk, stream);
}

extern "C" int pf_channel_stats_final(const double* partials, int B, int Np, int C, int nblk, float eps,
                                      float* scale, float* shift, void* stream) {
    PF_REQUIRE(partials && scale && shift);
    PF_REQUIRE_SHAPE(B > 0 && Np > 0 && C > 0 && C <= 256 && nblk > 0 && nblk <= (1 << 20));
    return PF_STATS_FINAL_LAUNCH(partials, B, Np, C, nblk, eps, scale, shift, stream);
}

extern "C" int pf_to_channel_last(const float* in, int c_total, int c_begin, int c, float* out,
                                  int ld_out, int off_out, int act, int B, int N, void* stream) {
    PF_REQUIRE(in && out && in != out);
    PF_REQUIRE_SHAPE(B > 0 && N > 0 && c > 0 && c_begin >= 0 && c_begin + c <= c_total);
    PF_REQUIRE(off_out >= 0 && off_out + c <= ld_out && act >= 0 && act <= 2);
    PfToNhwcArgs a; a.in = in; a.out = out; a.B = B; a.C_total = c_total; a.c_begin = c_begin; a.C = c;
    a.N = N; a.ld_out = ld_out; a.c_out_off = off_out; a.act = act;
    return PF_LAUNCH(to_nhwc, a, (long)B * N * c, stream);
}

extern "C" int pf_space_to_depth2(const float* in, int C, float* out, int ld_out, int B, int H, int W, void* stream) {
    PF_REQUIRE(in && out && in != out);
    PF_REQUIRE_SHAPE(B > 0 && C > 0 && H > 0 && W > 0 && (H & 1) == 0 && (W & 1) == 0 && ld_out >= 4 * C);
    PfS2dArgs a; a.in = in; a.out = out; a.B = B; a.C = C; a.H = H; a.W = W; a.ld_out = ld_out;
    return PF_LAUNCH(s2d, a, (long)B * (H / 2) * (W / 2) * 4 * C, stream);
}

extern "C" int pf_flow_metrics(const float* pred, const float* gt, float* epe, float* sd, int cosine, int B, int H, int W,
                               void* stream) {
    PF_REQUIRE(pred && gt && (epe || sd));
    PF_REQUIRE_SHAPE(B > 0 && H > 0 && W > 0);
    PfFlowMetricsArgs a; a.pred = pred; a.gt = gt; a.epe = epe; a.sd = sd; a.B = B; a.H = H; a.W = W; a.cosine = cosine;
    return PF_LAUNCH(flow_metrics, a, (long)B * H * W, stream);
}

// forward-backward check: the device build defines PF_FB_CHECK_LAUNCH (four pixels per thread where alignment allows)
#ifndef PF_FB_CHECK_LAUNCH
#define PF_FB_CHECK_LAUNCH(a, total, stream) PF_LAUNCH(fb_check, a, total, stream)
#endif
extern "C" int pf_fb_check(const float* flow_fw, const float* flow_bw, unsigned char* occ_fw, unsigned char* occ_bw, float* res_fw,
                           float* res_bw, int B, int H, int W, int metric, float alpha, float beta, void* stream) {
    PF_REQUIRE(flow_fw && flow_bw && occ_fw && occ_bw && res_fw && res_bw);
    PF_REQUIRE(flow_fw != flow_bw && res_fw != res_bw && occ_fw != occ_bw);
    PF_REQUIRE(res_fw != flow_fw && res_fw != flow_bw && res_bw != flow_fw && res_bw != flow_bw);
    PF_REQUIRE((const void*)occ_fw != flow_fw && (const void*)occ_fw != flow_bw && (const void*)occ_bw != flow_fw &&
               (const void*)occ_bw != flow_bw && (void*)occ_fw != res_fw && (void*)occ_fw != res_bw &&
               (void*)occ_bw != res_fw && (void*)occ_bw != res_bw);
    PF_REQUIRE(metric == PF_FB_PLANE || metric == PF_FB_SPHERE);
    PF_REQUIRE(alpha >= 0.f && alpha <= 3.0e38f && beta >= 0.f && beta <= 3.0e38f);       // (a NaN fails both comparisons)
    PF_REQUIRE_SHAPE(B > 0 && H > 1 && W > 1 && (long)H * W < (1L << 30));
    PfFbCheckArgs a; a.fw = flow_fw; a.bw = flow_bw; a.occ_fw = occ_fw; a.occ_bw = occ_bw; a.res_fw = res_fw; a.res_bw = res_bw;
    a.B = B; a.H = H; a.W = W; a.metric = metric; a.alpha = alpha; a.beta = beta;
    return PF_FB_CHECK_LAUNCH(a, 2L * B * H * W, stream);
}

// flow composition: the device build defines PF_FLOW_COMPOSE_LAUNCH (four pixels per thread where alignment allows)
#ifndef PF_FLOW_COMPOSE_LAUNCH
#define PF_FLOW_COMPOSE_LAUNCH(a, total, stream) PF_LAUNCH(flow_compose, a, total, stream)
#endif
extern "C" int pf_flow_compose(const pf_compose_job* jobs, int njobs, int B, int H, int W, void* stream) {
    PF_REQUIRE(jobs && njobs >= 1 && njobs <= PF_COMPOSE_MAX);
    PF_REQUIRE_SHAPE(B > 0 && H > 0 && W > 0 && (long)H * W < (1L << 30));
    PfComposeArgs a;
    for (int i = 0; i < PF_COMPOSE_MAX; ++i) {
        const pf_compose_job& j = jobs[i < njobs ? i : 0];
        PF_REQUIRE(j.f && j.g && j.out && j.out != j.g && (!j.state_out || j.state_out != j.occ_g));
        PF_REQUIRE((const void*)j.out != j.state_f && (const void*)j.out != j.occ_g && (void*)j.out != j.state_out &&
                   (const void*)j.state_out != j.f && (const void*)j.state_out != j.g);
        PfComposeJob& q = a.job[i];
        q.f = j.f; q.state_f = j.state_f; q.g = j.g; q.occ_g = j.occ_g; q.out = j.out; q.state_out = j.state_out;
    }
    for (int i = 0; i < njobs; ++i)             // the jobs run unordered: no output of one may be touched by another
        for (int k = 0; k < njobs; ++k) {
            if (k == i) continue;
            const PfComposeJob& w = a.job[i]; const PfComposeJob& o = a.job[k];
            const void* outs[2] = {w.out, w.state_out};
            const void* theirs[6] = {o.f, o.state_f, o.g, o.occ_g, o.out, o.state_out};
            for (const void* p : outs)
                for (const void* t : theirs) PF_REQUIRE(!p || p != t);
        }
    a.njobs = njobs; a.B = B; a.H = H; a.W = W;
    return PF_FLOW_COMPOSE_LAUNCH(a, (long)njobs * B * H * W, stream);
}

extern "C" int pf_track_points(float* pos, unsigned char* state, const float* flow, const unsigned char* occ, int B, int N,
                               int H, int W, void* stream) {
    PF_REQUIRE(pos && state && flow && (const void*)pos != flow && (const void*)state != occ);
    PF_REQUIRE_SHAPE(B > 0 && N > 0 && H > 0 && W > 0 && (long)H * W < (1L << 30));
    PfTrackArgs a; a.pos = pos; a.state = state; a.flow = flow; a.occ = occ; a.B = B; a.N = N; a.H = H; a.W = W;
    return PF_LAUNCH(track_points, a, (long)B * N, stream);
}

extern "C" int pf_track_grid(float* pos, int B, int H, int W, void* stream) {
    PF_REQUIRE(pos);
    PF_REQUIRE_SHAPE(B > 0 && H > 0 && W > 0 && (long)H * W < (1L << 30));
    PfTrackArgs a; a.pos = pos; a.state = nullptr; a.flow = nullptr; a.occ = nullptr; a.B = B; a.N = H * W; a.H = H; a.W = W;
    return PF_LAUNCH(track_grid, a, (long)B * H * W, stream);
}

extern "C" int pf_region_sums(const float* epe, const float* sd, const float* weight, const unsigned char* bits,
                              int nregions, double* partials, int nblk, int B, int N, void* stream) {
    PF_REQUIRE(epe && sd && bits && partials);
    PF_REQUIRE_SHAPE(B > 0 && N > 0 && nregions >= 1 && nregions <= 8 && nblk >= 1 && nblk <= 4096);
    PfRegionSumArgs a; a.epe = epe; a.sd = sd; a.weight = weight; a.bits = bits; a.partials = partials;
    a.B = B; a.N = N; a.R = nregions; a.nblk = nblk;
    return PF_REGION_SUM_LAUNCH(a, stream);
}

extern "C" int pf_seq_loss(const float* pred, const float* gt, const float* valid, const float* weight, float i_weight,
                           float max_flow, float* grad, double* partials, int nblk, int B, int N, void* stream) {
    PF_REQUIRE(pred && gt && valid && weight && partials);
    PF_REQUIRE_SHAPE(B > 0 && N > 0 && nblk >= 1 && nblk <= 4096);
    PfSeqLossArgs a; a.pred = pred; a.gt = gt; a.valid = valid; a.w = weight; a.grad = grad; a.partials = partials;
    a.B = B; a.N = N; a.nblk = nblk; a.i_weight = i_weight; a.max_flow = max_flow;
    return PF_SEQ_LOSS_LAUNCH(a, stream);
}

extern "C" int pf_seq_loss_batch(const float* const* preds, const float* gt, const float* valid, const float* weight,
                                 const float* i_weights, float max_flow, float* const* grads, double* partials, int nblk, int n,
                                 int B, int N, void* stream) {
    PF_REQUIRE(preds && gt && valid && weight && i_weights && partials);
    PF_REQUIRE_SHAPE(B > 0 && N > 0 && nblk >= 1 && nblk <= 4096 && n >= 1 && n <= PF_SEQ_LOSS_MAX);
    PfSeqLossBatch t;
    for (int i = 0; i < PF_SEQ_LOSS_MAX; ++i) {
        const int j = i < n ? i : 0;
        PF_REQUIRE(preds[j] != nullptr);
        t.pred[i] = preds[j]; t.grad[i] = grads ? grads[j] : nullptr; t.i_weight[i] = i_weights[j];
    }
    t.common.pred = nullptr; t.common.grad = nullptr; t.common.i_weight = 0.f;
    t.common.gt = gt; t.common.valid = valid; t.common.w = weight; t.common.partials = partials;
    t.common.B = B; t.common.N = N; t.common.nblk = nblk; t.common.max_flow = max_flow;
    t.n = n;
    return PF_SEQ_LOSS_BATCH_LAUNCH(t, stream);
}

extern "C" int pf_sum_squares(const float* x, long n, double* partials, int nblk, void* stream) {
    PF_REQUIRE(x && partials);
    PF_REQUIRE_SHAPE(n > 0 && nblk >= 1 && nblk <= 65536);
    PfSumSqArgs a; a.x = x; a.partials = partials; a.n = n; a.nblk = nblk;
    return PF_SUMSQ_LAUNCH(a, stream);
}

extern "C" int pf_adamw_step(float* p, const float* g, float* m, float* v, long n, double lr, float beta1, float beta2,
                             float eps, double weight_decay, int step, float grad_scale, void* stream) {
    PF_REQUIRE(p && g && m && v && p != g && m != v);
    PF_REQUIRE_SHAPE(n > 0 && step >= 1 && beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f);
    PfAdamWArgs a; a.p = p; a.g = g; a.m = m; a.v = v; a.n = n;
    a.b1 = beta1; a.b2 = beta2; a.eps = eps; a.gscale = grad_scale;
    // python-float (double) scalar arithmetic of torch's single-tensor AdamW, rounded to fp32 once
    a.decay = (float)(1.0 - (double)lr * (double)weight_decay);
    a.step_size = (float)((double)lr / (1.0 - pow((double)beta1, (double)step)));
    a.sqrt_bc2 = (float)sqrt(1.0 - pow((double)beta2, (double)step));
    return PF_LAUNCH(adamw, a, n, stream);
}

extern "C" int pf_adamw_step_dev(float* p, const float* g, float* m, float* v, long n, float beta1, float beta2, float eps,
                                 const float* hyper, void* stream) {
    PF_REQUIRE(p && g && m && v && hyper && p != g && m != v);
    PF_REQUIRE_SHAPE(n > 0 && beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f);
    PfAdamWDevArgs a; a.p = p; a.g = g; a.m = m; a.v = v; a.n = n; a.b1 = beta1; a.b2 = beta2; a.eps = eps; a.hyper = hyper;
    return PF_LAUNCH(adamw_dev, a, n, stream);
}

extern "C" int pf_warp_gcorr_bwd(const float* f1, const float* f2, const float* coords, int add_grid, const float* d_flaw,
                                 int ld_d, int off_d, float* d_f1, float* d_f2, int B, int H8, int W8, int C, void* stream) {
    PF_REQUIRE(f1 && f2 && coords && d_flaw && d_f1 && d_f2 && d_f1 != d_f2);
    PF_REQUIRE_SHAPE(B > 0 && H8 > 1 && W8 > 1 && C > 0 && C % 4 == 0);
    PF_REQUIRE(off_d >= 0 && off_d + 4 <= ld_d);
    PfWarpGcorrBwdArgs a; a.f1 = f1; a.f2 = f2; a.coords = coords; a.d_flaw = d_flaw; a.ld_d = ld_d; a.off_d = off_d;
    a.d_f1 = d_f1; a.d_f2 = d_f2; a.B = B; a.H = H8; a.W = W8; a.C = C; a.add_grid = add_grid;
    return PF_LAUNCH(warp_gcorr_bwd, a, (long)B * H8 * W8 * C, stream);
}

extern "C" int pf_upsample_flow_bwd(const float* coords1, const float* mask, int ld, const float* g, float* d_mask, int ld_d,
                                    float* d_flow, int B, int H8, int W8, void* stream) {
    PF_REQUIRE(coords1 && mask && g && d_mask && d_flow && mask != d_mask);
    PF_REQUIRE_SHAPE(B > 0 && H8 > 0 && W8 > 0 && ld >= 576 && ld_d >= 576);
    PfUpsampleBwdArgs a; a.coords1 = coords1; a.mask = mask; a.g = g; a.d_mask = d_mask; a.d_flow = d_flow;
    a.B = B; a.H = H8; a.W = W8; a.ld = ld; a.ld_d = ld_d;
    return PF_UPSAMPLE_BWD_LAUNCH(a, (long)B * 64 * H8 * W8, stream);
}

extern "C" int pf_pyramid_bwd(float* g0, const float* g1, const float* g2, const float* g3, int B, int H8, int W8,
                              void* stream) {
    PF_REQUIRE(g0 && g1 && g2 && g3);
    PF_REQUIRE_SHAPE(B > 0 && (H8 >> 3) >= 1 && (W8 >> 3) >= 1);
    PfPyramidBwdArgs a; a.g0 = g0; a.g1 = g1; a.g2 = g2; a.g3 = g3; a.rows = (long)B * H8 * W8; a.H = H8; a.W = W8;
    return PF_LAUNCH(pyramid_bwd, a, a.rows * H8 * W8, stream);
}

extern "C" int pf_norm_bwd(const float* dy, const float* x, const float* scale, const float* shift, int relu, int instance,
                           double* partials, int nblk, float* coef, float* dx, int B, int Np, int C, void* stream) {
    PF_REQUIRE(dy && x && scale && shift && dx && dx != x);
    PF_REQUIRE(!instance || (partials && coef && nblk > 0));
    PF_REQUIRE_SHAPE(B > 0 && Np > 0 && C > 0 && (!instance || nblk <= Np));
    PfNormBwdArgs a; a.dy = dy; a.x = x; a.s = scale; a.t = shift; a.part = partials; a.coef = coef; a.dx = dx;
    a.B = B; a.Np = Np; a.C = C; a.nblk = nblk; a.relu = relu; a.instance = instance;
    if (instance) {
        int rc = PF_LAUNCH(norm_bwd_partial, a, (long)B * nblk * C, stream);
        if (rc != PF_OK) return rc;
#ifdef PF_PAIR_FINAL_LAUNCH
        rc = PF_PAIR_FINAL_LAUNCH(partials, B, nblk, C, 0, Np, coef, nullptr, 0, stream);
#else
        rc = PF_LAUNCH(norm_bwd_final, a, (long)B * C, stream);
#endif
        if (rc != PF_OK) return rc;
    }
    return PF_LAUNCH(norm_bwd_apply, a, (long)B * Np * C, stream);
}

extern "C" int pf_add_relu(const float* x, const float* y, float* out, long n, void* stream) {
    PF_REQUIRE(x && y && out && n > 0);
    PfAddReluArgs a; a.x = x; a.y = y; a.out = out; a.n = n;
    return PF_LAUNCH(add_relu, a, (n + 3) / 4, stream);
}

extern "C" int pf_relu_mask(const float* g, const float* fwd_out, float* dx, long n, void* stream) {
    PF_REQUIRE(g && fwd_out && dx && n > 0);
    PfAddReluArgs a; a.x = g; a.y = fwd_out; a.out = dx; a.n = n;
    return PF_LAUNCH(relu_mask, a, (n + 3) / 4, stream);
}

extern "C" int pf_bn_frozen_fwd(const float* x, const float* gamma, const float* beta, const float* mean, const float* var,
                                float eps, int relu, float* out, long rows, int C, void* stream) {
    PF_REQUIRE(x && gamma && beta && mean && var && out);
    PF_REQUIRE_SHAPE(rows > 0 && C > 0 && eps > 0.f);
    PfBnArgs a{}; a.x = x; a.gamma = gamma; a.beta = beta; a.mean = mean; a.var = var; a.out = out;
    a.eps = eps; a.rows = rows; a.C = C; a.relu = relu;
    return PF_LAUNCH(bn_fwd, a, rows * C, stream);
}

extern "C" int pf_bn_frozen_bwd(const float* dy, const float* x, const float* gamma, const float* beta, const float* mean,
                                const float* var, float eps, int relu, double* partials, int nblk, float* dx,
                                float* dgamma, float* dbeta, int accumulate, long rows, int C, void* stream) {
    PF_REQUIRE(dy && x && gamma && beta && mean && var && partials && dx && dgamma && dbeta && dx != x);
    PF_REQUIRE_SHAPE(rows > 0 && C > 0 && eps > 0.f && nblk > 0 && (long)nblk <= rows);
    PfBnArgs a{}; a.x = x; a.dy = dy; a.gamma = gamma; a.beta = beta; a.mean = mean; a.var = var; a.out = dx;
    a.part = partials; a.dgamma = dgamma; a.dbeta = dbeta; a.eps = eps; a.rows = rows; a.C = C; a.nblk = nblk; a.relu = relu;
    a.accumulate = accumulate;
    int rc = PF_LAUNCH(bn_bwd_partial, a, (long)nblk * C, stream);
    if (rc != PF_OK) return rc;
#ifdef PF_PAIR_FINAL_LAUNCH
    rc = PF_PAIR_FINAL_LAUNCH(partials, 1, nblk, C, 1, 0, dbeta, dgamma, accumulate, stream);
#else
    rc = PF_LAUNCH(bn_bwd_final, a, (long)C, stream);
#endif
    if (rc != PF_OK) return rc;
    return PF_LAUNCH(bn_bwd_apply, a, rows * C, stream);
}

extern "C" int pf_gru_q_bwd(const float* dh_new, int ld_dhn, const float* z, int ld_z, const float* q, int ld_q,
                            const float* h, int ld_h, float* dq_pre, int ld_dq, float* dz, int ld_dz,
                            float* dh, int ld_dh, long rows, int C, void* stream) {
    PF_REQUIRE(dh_new && z && q && h && dq_pre && dz && dh);
    PF_REQUIRE_SHAPE(rows > 0 && C > 0 && ld_dhn >= C && ld_z >= C && ld_q >= C && ld_h >= C && ld_dq >= C && ld_dz >= C && ld_dh >= C);
    PfGruQBwdArgs a; a.dhn = dh_new; a.z = z; a.q = q; a.h = h; a.dq_pre = dq_pre; a.dz = dz; a.dh = dh;
    a.ld_dhn = ld_dhn; a.ld_z = ld_z; a.ld_q = ld_q; a.ld_h = ld_h; a.ld_dq = ld_dq; a.ld_dz = ld_dz; a.ld_dh = ld_dh; a.C = C;
    return PF_LAUNCH(gru_q_bwd, a, rows * C, stream);
}

extern "C" int pf_gru_dx_finish(const float* f1, int ld_f1, const float* f2, int ld_f2, const float* x, int ld_x,
                                float* d_inp, int ld_dinp, float* d_out, int ld_dout, long rows, int C, int wout, void* stream) {
    PF_REQUIRE(f1 && f2 && x && d_inp && d_out);
    PF_REQUIRE_SHAPE(rows > 0 && C > 0 && wout > 0 && ld_f1 >= C + wout && ld_f2 >= C + wout && ld_x >= C + wout && ld_dinp >= C && ld_dout >= wout);
    PfGruDxArgs a; a.f1 = f1; a.f2 = f2; a.x = x; a.d_inp = d_inp; a.d_out = d_out;
    a.ld_f1 = ld_f1; a.ld_f2 = ld_f2; a.ld_x = ld_x; a.ld_dinp = ld_dinp; a.ld_dout = ld_dout; a.C = C; a.wout = wout;
    return PF_LAUNCH(gru_dx_finish, a, rows * (C + wout), stream);
}

extern "C" int pf_gru_zr_bwd(const float* dz, int ld_dz, const float* d_rh, int ld_drh, const float* z, int ld_z,
                             const float* r, int ld_r, const float* h, int ld_h, float* dzr_pre, int ld_dzr,
                             float* dh, int ld_dh, long rows, int C, void* stream) {
    PF_REQUIRE(dz && d_rh && z && r && h && dzr_pre && dh);
    PF_REQUIRE_SHAPE(rows > 0 && C > 0 && ld_dz >= C && ld_drh >= C && ld_z >= C && ld_r >= C && ld_h >= C && ld_dzr >= 2 * C && ld_dh >= C);
    PfGruZrBwdArgs a; a.dz = dz; a.d_rh = d_rh; a.z = z; a.r = r; a.h = h; a.dzr_pre = dzr_pre; a.dh = dh;
    a.ld_dz = ld_dz; a.ld_drh = ld_drh; a.ld_z = ld_z; a.ld_r = ld_r; a.ld_h = ld_h; a.ld_dzr = ld_dzr; a.ld_dh = ld_dh; a.C = C;
    return PF_LAUNCH(gru_zr_bwd, a, rows * C, stream);
}

extern "C" int pf_dccl_combine_bwd(const float* d_corr, int ld_in, const float* g_back, float* d_raw, int ld,
                                   int B, int H8, int W8, void* stream) {
    PF_REQUIRE(d_corr && g_back && d_raw && d_corr != d_raw);
    PF_REQUIRE_SHAPE(B > 0 && H8 > 1 && W8 > 1 && ld >= PF_CORR_CH && ld_in >= PF_CORR_CH);
    PfCombineBwdArgs a; a.d_corr = d_corr; a.g_back = g_back; a.d_raw = d_raw; a.B = B; a.H = H8; a.W = W8;
    a.ld_in = ld_in; a.ld = ld;
    return PF_LAUNCH(combine_bwd, a, (long)B * H8 * W8 * PF_CORR_CH, stream);
}

extern "C" int pf_dccl_lookup_bwd(const float* coords, const float* g_w2c, const float* d_own, float* d_raw, int ld,
                                  float* own0, float* own1, float* own2, float* own3,
                                  float* oth0, float* oth1, float* oth2, float* oth3,
                                  int B, int H8, int W8, int clear_raw, void* stream) {
    PF_REQUIRE(coords && g_w2c && d_own && d_raw && own0 && own1 && own2 && own3 && oth0 && oth1 && oth2 && oth3);
    PF_REQUIRE_SHAPE(B > 0 && (H8 >> 3) >= 2 && (W8 >> 3) >= 2 && ld >= PF_CORR_CH);
    PfLookupBwdArgs a; a.coords = coords; a.g_w2c = g_w2c; a.d_own = d_own; a.d_raw = d_raw; a.ld = ld;
    a.g_own[0] = own0; a.g_own[1] = own1; a.g_own[2] = own2; a.g_own[3] = own3;
    a.g_other[0] = oth0; a.g_other[1] = oth1; a.g_other[2] = oth2; a.g_other[3] = oth3;
    a.B = B; a.H = H8; a.W = W8; a.clear_raw = clear_raw ? d_raw : nullptr;
    return PF_LOOKUP_BWD_LAUNCH(a, (long)B * H8 * W8 * PF_CORR_CH, stream);
}

extern "C" int pf_to_nchw(const float* in, int ld_in, int off_in, int c, float* out, int B, int N,
                          void* stream) {
    PF_REQUIRE(in && out && in != out);
    PF_REQUIRE_SHAPE(B > 0 && N > 0 && c > 0 && off_in >= 0 && off_in + c <= ld_in);
    PfToNchwArgs a; a.in = in; a.out = out; a.B = B; a.C = c; a.N = N; a.ld_in = ld_in; a.c_in_off = off_in;
    return PF_LAUNCH(to_nchw, a, (long)B * c * N, stream);
}

// pf_warp_gcorr: validation shared; the launch itself differs (wavefront kernel on device)
static inline int pf_warp_gcorr_fill(PfWarpGcorrArgs& a, const float* f1, const float* f2,
                                     const float* coords, int add_grid, float* dst, int dst_ld,
                                     int dst_off, int B, int H8, int W8, int C) {
    PF_REQUIRE(f1 && f2 && coords && dst);
    PF_REQUIRE_SHAPE(B > 0 && H8 > 1 && W8 > 1 && C > 0 && C % 4 == 0);
    PF_REQUIRE(dst_off >= 0 && dst_off + 4 <= dst_ld);
    a.f1 = f1; a.f2 = f2; a.coords = coords; a.dst = pf_dst(dst, dst_ld, dst_off);
    a.B = B; a.H = H8; a.W = W8; a.C = C; a.add_grid = add_grid;
    return PF_OK;
}

#if !defined(__HIPCC__)
// Host build (tests/emu): the f16-map forms of the motion-input producers as their fp32 forms into a temporary + pf_f16_put
// (the device kernels write the same values straight from registers).  The fused combine + 1x1 has no host statement in either
// operand form.
#include <stdlib.h>
extern "C" int pf_conf_stem_f16(const float* in, int ld_in, int off_in, const float* w1, const float* b1,
                                const float* w2, const float* b2, float* out, int ld_out, int off_out,
                                void* out_f16, int lds_out, int B, int H8, int W8, void* stream) {
    PF_REQUIRE(out || out_f16);
    PF_REQUIRE_SHAPE(B > 0 && H8 > 0 && W8 > 0 && off_out >= 0 && (!out_f16 || off_out + 16 <= lds_out * 64));
    const long rows = (long)B * H8 * W8;
    float* t = (float*)malloc(sizeof(float) * rows * 16);
    if (!t) return PF_ERR_BAD_ARG;
    int rc = pf_conf_stem(in, ld_in, off_in, w1, b1, w2, b2, t, 16, 0, nullptr, 0, B, H8, W8, stream);
    for (long r = 0; rc == PF_OK && r < rows; ++r)
        for (int c = 0; c < 16; ++c) {
            if (out) out[r * ld_out + off_out + c] = t[r * 16 + c];
            if (out_f16) pf_f16_put(out_f16, r, lds_out, off_out + c, t[r * 16 + c]);
        }
    free(t);
    return rc;
}

extern "C" int pf_motion_prep_f16(const float* c1a, const float* c1b, const float* g_w2c, const float* g_c2w,
                                  const float* f1a, const float* f2a, float* flow4_a, float* flow2_b,
                                  float* xa, int xa_ld, int xa_off, float* xb, int xb_ld, int xb_off,
                                  void* xa_f16, int xa_lds, void* xb_f16, int xb_lds,
                                  float* conf, int conf_ld, int B, int H8, int W8, int C, void* stream) {
    PF_REQUIRE_SHAPE(B > 0 && H8 > 0 && W8 > 0);
    PF_REQUIRE(!xa_f16 || (xa_off >= 0 && xa_off + 4 <= xa_lds * 64));
    PF_REQUIRE(!xb_f16 || (xb_off >= 0 && xb_off + 2 <= xb_lds * 64));
    const long rows = (long)B * H8 * W8;
    float* t = (float*)malloc(sizeof(float) * rows * 6);      // [rows][4] tails of xa, then [rows][2] of xb
    if (!t) return PF_ERR_BAD_ARG;
    int rc = pf_motion_prep(c1a, c1b, g_w2c, g_c2w, f1a, f2a, flow4_a, flow2_b, t, 4, 0, t + rows * 4, 2, 0,
                            nullptr, 0, nullptr, 0, conf, conf_ld, B, H8, W8, C, stream);
    for (long r = 0; rc == PF_OK && r < rows; ++r) {
        for (int c = 0; c < 4; ++c) {
            if (xa) xa[r * xa_ld + xa_off + c] = t[r * 4 + c];
            if (xa_f16) pf_f16_put(xa_f16, r, xa_lds, xa_off + c, t[r * 4 + c]);
        }
        for (int c = 0; c < 2; ++c) {
            if (xb) xb[r * xb_ld + xb_off + c] = t[rows * 4 + r * 2 + c];
            if (xb_f16) pf_f16_put(xb_f16, r, xb_lds, xb_off + c, t[rows * 4 + r * 2 + c]);
        }
    }
    free(t);
    return rc;
}

extern "C" int pf_dccl_combine_conv1x1_f16(const pf_combine_conv_desc*, int, int, int, int, void*) { return PF_ERR_BAD_SHAPE; }
#endif

// ---- flow rendering (DESIGN.md section 13): order statistic, colour coding, cyclic warp ----------------------------------------
#if !defined(__HIPCC__)
// Host build (tests/emu): a select pass as its host statement (the choice of the previous pass per image, then the counts element
// by element); the device build defines these macros as the workgroup kernels of pf_elem_kernels.hip and never falls back to this.
static int pf_os_pass_host(PfOrderStatArgs a, int pass, void* stream) {
    a.pass = pass;
    if (pass > 0)
        for (int b = 0; b < a.B; ++b) pf_os_select_image(a, b, pass);
    return PF_LAUNCH(os_hist, a, (long)a.B * a.n, stream);
}
static int pf_os_final_host(const PfOrderStatArgs& a, void*) {
    for (int b = 0; b < a.B; ++b) pf_os_select_image(a, b, 3);
    return PF_OK;
}
static int pf_render_len_host(const PfOrderStatArgs& o, const PfRenderArgs& r, void* stream) {
    const int rc = PF_LAUNCH(render_len, r, (long)r.B * r.H * r.W, stream);
    return rc == PF_OK ? pf_os_pass_host(o, 0, stream) : rc;
}
static int pf_render_color_host(const PfOrderStatArgs& o, const PfRenderArgs& r, void* stream) {
    const int rc = pf_os_final_host(o, stream);
    return rc == PF_OK ? PF_LAUNCH(render_color, r, (long)r.B * r.H * r.W, stream) : rc;
}
static int pf_masked_mean_host(const PfMaskedMeanArgs& a, void*) {
    const int chunk = (a.N + a.nblk - 1) / a.nblk;
    for (int b = 0; b < a.B; ++b)
        for (int k = 0; k < a.nblk; ++k) {
            double s = 0.0, c = 0.0;
            for (int n = k * chunk; n < (k + 1) * chunk && n < a.N; ++n)
                if (!a.mask || a.mask[(long)b * a.N + n] == 0) { s += (double)a.x[(long)b * a.N + n]; c += 1.0; }
            a.partials[((long)b * a.nblk + k) * 2] = s; a.partials[((long)b * a.nblk + k) * 2 + 1] = c;
        }
    return PF_OK;
}
#define PF_OS_PASS_LAUNCH(a, pass, stream) pf_os_pass_host(a, pass, stream)
#define PF_OS_FINAL_LAUNCH(a, stream) pf_os_final_host(a, stream)
#define PF_RENDER_LEN_LAUNCH(o, r, stream) pf_render_len_host(o, r, stream)
#define PF_RENDER_COLOR_LAUNCH(o, r, stream) pf_render_color_host(o, r, stream)
#define PF_MASKED_MEAN_LAUNCH(a, stream) pf_masked_mean_host(a, stream)
#endif

extern "C" long pf_order_stat_scratch_bytes(int B, long n) {
    if (B <= 0 || B > PF_MAX_IMAGES || n <= 0 || n >= (1L << 31)) return PF_ERR_BAD_SHAPE;
    return 4L * B * (PF_OS_HIST + 4);
}

static inline void pf_os_fill(PfOrderStatArgs& a, const float* x, float* out, void* scratch, int B, long n, long k) {
    a.x = x; a.out = out; a.hist = (unsigned*)scratch; a.state = a.hist + (long)B * PF_OS_HIST;
    a.n = n; a.k = k; a.B = B; a.pass = 0;
}

extern "C" int pf_order_stat(const float* x, float* out, void* scratch, long scratch_bytes, int B, long n, long k, void* stream) {
    PF_REQUIRE(x && out && scratch && (const void*)x != (const void*)out);
    PF_REQUIRE_SHAPE(B > 0 && B <= PF_MAX_IMAGES && n > 0 && n < (1L << 31));
    PF_REQUIRE(k >= 0 && k < n && scratch_bytes >= pf_order_stat_scratch_bytes(B, n) && ((unsigned long)scratch & 3ul) == 0);
    PfOrderStatArgs a; pf_os_fill(a, x, out, scratch, B, n, k);
    int rc = PF_LAUNCH(os_zero, a, (long)B * (PF_OS_HIST + 4), stream);
    for (int p = 0; p < 3 && rc == PF_OK; ++p) rc = PF_OS_PASS_LAUNCH(a, p, stream);
    if (rc == PF_OK) rc = PF_OS_FINAL_LAUNCH(a, stream);
    return rc;
}

extern "C" long pf_flow_render_scratch_bytes(int B, int H, int W) {
    if (B <= 0 || B > PF_MAX_IMAGES || H <= 1 || W <= 1 || (long)H * W >= (1L << 30)) return PF_ERR_BAD_SHAPE;
    return 4L * B * H * W + 4L * B + pf_order_stat_scratch_bytes(B, (long)H * W);
}

extern "C" int pf_flow_render(const float* flow, unsigned char* out, void* scratch, long scratch_bytes, int B, int H, int W,
                              int mode, double percentile, int layout, int bgr, void* stream) {
    PF_REQUIRE(flow && out && scratch && (const void*)flow != (const void*)out);
    PF_REQUIRE(mode == PF_RENDER_OMNI || mode == PF_RENDER_PLANE);
    PF_REQUIRE(layout == PF_LAYOUT_HWC || layout == PF_LAYOUT_CHW);
    PF_REQUIRE(bgr == 0 || bgr == 1);
    PF_REQUIRE(percentile >= 0.0 && percentile <= 1.0);                    // (a NaN fails both comparisons)
    PF_REQUIRE_SHAPE(B > 0 && B <= PF_MAX_IMAGES && H > 1 && W > 1 && (long)H * W < (1L << 30));
    PF_REQUIRE(scratch_bytes >= pf_flow_render_scratch_bytes(B, H, W) && ((unsigned long)scratch & 3ul) == 0);
    const long N = (long)H * W;
    long k = mode == PF_RENDER_PLANE ? N - 1 : (long)(percentile * (double)N);
    if (k > N - 1) k = N - 1;
    PfRenderArgs r; r.flow = flow; r.len = (float*)scratch; r.out = out; r.B = B; r.H = H; r.W = W;
    r.mode = mode; r.planar = layout == PF_LAYOUT_CHW; r.bgr = bgr;
    float* clip = r.len + (long)B * N;
    r.clip = clip;
    PfOrderStatArgs a; pf_os_fill(a, r.len, clip, clip + B, B, N, k);
    int rc = PF_LAUNCH(os_zero, a, (long)B * (PF_OS_HIST + 4), stream);
    if (rc == PF_OK) rc = PF_RENDER_LEN_LAUNCH(a, r, stream);
    if (rc == PF_OK) rc = PF_OS_PASS_LAUNCH(a, 1, stream);
    if (rc == PF_OK) rc = PF_OS_PASS_LAUNCH(a, 2, stream);
    if (rc == PF_OK) rc = PF_RENDER_COLOR_LAUNCH(a, r, stream);
    return rc;
}

extern "C" int pf_cycle_warp(const float* x, const float* flo, const float* ref, float* out, float* err, int B, int C, int H,
                             int W, void* stream) {
    PF_REQUIRE(x && flo && out && out != x && out != flo && out != ref);
    PF_REQUIRE((err != nullptr) == (ref != nullptr) && err != out && (!err || (err != x && err != flo && err != ref)));
    PF_REQUIRE_SHAPE(B > 0 && C > 0 && H > 1 && W > 1 && (long)H * W < (1L << 30));
    PfCycleWarpArgs a; a.x = x; a.flo = flo; a.ref = ref; a.out = out; a.err = err; a.B = B; a.C = C; a.H = H; a.W = W;
    return PF_LAUNCH(cycle_warp, a, (long)B * H * W, stream);
}

extern "C" int pf_masked_mean(const float* x, const unsigned char* mask, float* out, void* scratch, long scratch_bytes, int B,
                              int N, void* stream) {
    PF_REQUIRE(x && out && scratch && out != x);
    PF_REQUIRE_SHAPE(B > 0 && B <= PF_MAX_IMAGES && N > 0 && N < (1 << 30));
    PF_REQUIRE(scratch_bytes >= 16L * B * PF_MM_BLOCKS && ((unsigned long)scratch & 7ul) == 0);
    PfMaskedMeanArgs a; a.x = x; a.mask = mask; a.partials = (double*)scratch; a.out = out; a.B = B; a.N = N;
    a.nblk = N < PF_MM_BLOCKS * 256 ? (N + 255) / 256 : PF_MM_BLOCKS;
    const int rc = PF_MASKED_MEAN_LAUNCH(a, stream);
    return rc == PF_OK ? PF_LAUNCH(masked_mean_final, a, (long)B, stream) : rc;
}
