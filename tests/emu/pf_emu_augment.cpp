// Host emulation of pf_augment_360 / pf_augment_convert -- TEST INFRASTRUCTURE ONLY (its own library, libpf_emu_augment.so).
// The per-pixel arithmetic is prior-flow_amd/csrc/pf_augment.h, the file the device kernels compile; the passes are restated as
// plain loops: the L sums, the main pass (chain, roll, flow, valid, image 2's channel sums), the eraser in rolled coordinates.
// The product never loads this library.
#include "pf_augment.h"

extern "C" long pf_augment_scratch_bytes(int B) { return pf_augment_scratch_bytes_impl(B); }

extern "C" int pf_augment_360(const unsigned char* img1, const unsigned char* img2, const float* flow, const int* params,
                              float* image1, float* image2, float* flow_gt, float* valid, void* scratch, long scratch_bytes,
                              int B, int H, int W, void*) {
    const int rc = pf_augment_check(img1, img2, flow, params, image1, image2, flow_gt, valid, scratch, scratch_bytes, B, H, W);
    if (rc != PF_OK) return rc;
    const long N = (long)H * W;
    unsigned long long* sums = reinterpret_cast<unsigned long long*>(scratch);
    const unsigned char* img[2] = {img1, img2};
    float* out[2] = {image1, image2};
    for (long i = 0; i < (long)B * PF_AUG_SUMS; ++i) sums[i] = 0ull;
    for (int b = 0; b < B; ++b) {
        const int* row = params + (long)b * PF_AUG_ROW;
        unsigned long long* s = sums + (long)b * PF_AUG_SUMS;
        for (int k = 0; k < 2; ++k) {                       // the contrast pass
            const int second = pf_aug_second(row, k);
            const PfAugSet set = pf_aug_set(row, second);
            const int upto = pf_aug_contrast_at(set);
            if (upto < 0) continue;
            const unsigned char* src = img[k] + (long)b * N * 3;
            unsigned long long acc = 0;
            for (long n = 0; n < N; ++n) acc += (unsigned)pf_aug_luma(pf_aug_chain(pf_aug_load(src + n * 3), set, 0, upto));
            s[second] += acc;
        }
        const int asym_colour = row[PF_AUG_MODE] & PF_AUG_ASYM_COLOUR;
        for (int k = 0; k < 2; ++k) {                       // the main pass, images
            const int second = pf_aug_second(row, k);
            const PfAugSet set = pf_aug_set(row, second);
            const int mean = pf_aug_mean(s[second], (unsigned long long)N * (asym_colour ? 1 : 2));
            const int r = pf_aug_wrap(row[k ? PF_AUG_R2 : PF_AUG_R1], W);
            const unsigned char* src = img[k] + (long)b * N * 3;
            float* o = out[k] + (long)b * 3 * N;
            unsigned long long sr = 0, sg = 0, sb = 0;
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x) {
                    int xs = x - r;
                    if (xs < 0) xs += W;
                    const PfAugRgb c = pf_aug_chain(pf_aug_load(src + ((long)y * W + xs) * 3), set, mean, 4);
                    const long n = (long)y * W + x;
                    o[n] = (float)c.r; o[N + n] = (float)c.g; o[2 * N + n] = (float)c.b;
                    sr += c.r; sg += c.g; sb += c.b;
                }
            if (k == 1 && row[PF_AUG_NRECT] > 0) { s[2] += sr; s[3] += sg; s[4] += sb; }
        }
        {                                                   // the main pass, flow
            const int asym = (row[PF_AUG_MODE] & PF_AUG_ASYM_ROLL) ? 1 : 0;
            const int r1 = row[PF_AUG_R1], r2 = row[PF_AUG_R2], r = pf_aug_wrap(r1, W);
            const float* f = flow + (long)b * N * 2;
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x) {
                    int xs = x - r;
                    if (xs < 0) xs += W;
                    const float* p = f + ((long)y * W + xs) * 2;
                    const PfAugFlow q = pf_aug_flow(p[0], p[1], W, asym, r1, r2);
                    const long n = (long)y * W + x;
                    flow_gt[(long)b * 2 * N + n] = q.u; flow_gt[(long)b * 2 * N + N + n] = q.v; valid[(long)b * N + n] = q.valid;
                }
        }
        for (int k = 0; k < 2; ++k) {                       // the eraser
            int x0, y0, w, h;
            if (!pf_aug_rect(row, k, H, W, x0, y0, w, h)) continue;
            const float m[3] = {(float)(s[2] / (unsigned long long)N), (float)(s[3] / (unsigned long long)N),
                                (float)(s[4] / (unsigned long long)N)};
            const int r = pf_aug_wrap(row[PF_AUG_R2], W);
            float* o = image2 + (long)b * 3 * N;
            for (int i = 0; i < w * h; ++i) {
                const int yy = y0 + i / w;
                int xx = x0 + i % w + r;
                if (xx >= W) xx -= W;
                for (int c = 0; c < 3; ++c) o[c * N + (long)yy * W + xx] = m[c];
            }
        }
    }
    return PF_OK;
}

extern "C" int pf_augment_convert(const unsigned char* in, unsigned char* out, long n, int mode, void*) {
    if (!in || !out || in == out || (mode != 0 && mode != 1)) return PF_ERR_BAD_ARG;
    if (n < 1 || n >= (1L << 30)) return PF_ERR_BAD_SHAPE;
    for (long i = 0; i < n; ++i) {
        const PfAugRgb c = pf_aug_load(in + i * 3);
        const PfAugRgb o = mode ? pf_aug_hsv_to_rgb(c.r, c.g, c.b) : pf_aug_rgb_to_hsv(c);
        out[i * 3] = (unsigned char)o.r; out[i * 3 + 1] = (unsigned char)o.g; out[i * 3 + 2] = (unsigned char)o.b;
    }
    return PF_OK;
}
extern "C" const char* pf_version(void) { return "priorflow augmentation host emulation (tests only)"; }
