// Training augmentation for the 360-degree sets on the device: FlowAugmentor_360
// (core/utils/augmentor.py:210-316) and the loader steps around it (core/datasets.py:137-159) as four launches.
//
//   pf_aug_zero_kernel      the per-sample integer sums
//   pf_aug_contrast_kernel  the steps before each sample's contrast step, then the sum of L (both images in the symmetric mode)
//   pf_aug_main_kernel      the whole chain with int(mean + 0.5) from those sums, written as fp32 planes at the rolled position;
//                           image 2's channel sums; the flow's wrap, roll, asymmetric correction and `valid` (grid.y = 2)
//   pf_aug_erase_kernel     the eraser rectangles in rolled coordinates, filled with sum // (H W)
//
// Every sum is an integer: reduced in the wave, across the waves through LDS, then one 64-bit atomic per workgroup and quantity,
// so the result does not depend on the order of the adds.  The per-pixel arithmetic is pf_augment.h.
#include "pf_augment.h"

namespace {
constexpr int kBlock = 256;
constexpr int kMaxBlocks = 1024;

struct PfAugArgs {
    const unsigned char* img[2];
    const float* flow;
    const int* params;
    float* out[2];
    float* oflow;
    float* ovalid;
    unsigned long long* sums;
    int B, H, W;
};

__global__ void pf_aug_zero_kernel(unsigned long long* sums, int n) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) sums[i] = 0ull;
}

// sum of v over the workgroup, valid in thread 0
__device__ __forceinline__ unsigned long long pf_aug_block_sum(unsigned v, unsigned long long* red) {
    unsigned long long s = v;
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    const unsigned long long t = threadIdx.x == 0 ? red[0] + red[1] + red[2] + red[3] : 0ull;
    __syncthreads();
    return t;
}

// twelve bytes (four pixels) from p: three dwords when p is 4-byte aligned, bytes otherwise
__device__ __forceinline__ void pf_aug_load4(const unsigned char* p, PfAugRgb (&c)[4]) {
    if (((uintptr_t)p & 3) == 0) {
        const unsigned* q = reinterpret_cast<const unsigned*>(p);
        const unsigned a = q[0], b = q[1], d = q[2];
        c[0].r = a & 255; c[0].g = (a >> 8) & 255; c[0].b = (a >> 16) & 255;
        c[1].r = a >> 24; c[1].g = b & 255; c[1].b = (b >> 8) & 255;
        c[2].r = (b >> 16) & 255; c[2].g = b >> 24; c[2].b = d & 255;
        c[3].r = (d >> 8) & 255; c[3].g = (d >> 16) & 255; c[3].b = d >> 24;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) c[j] = pf_aug_load(p + 3 * j);
    }
}

// grid (blocks, 2 images, B)
__global__ void __launch_bounds__(kBlock) pf_aug_contrast_kernel(const PfAugArgs a) {
    __shared__ unsigned long long red[4];
    const int b = blockIdx.z, img = blockIdx.y;
    const int* row = a.params + (long)b * PF_AUG_ROW;
    const int second = pf_aug_second(row, img);
    const PfAugSet s = pf_aug_set(row, second);
    const int upto = pf_aug_contrast_at(s);
    if (upto < 0) return;                                   // the whole workgroup: nothing reads this sum
    const long N = (long)a.H * a.W;
    const unsigned char* src = a.img[img] + (long)b * N * 3;
    const long stride = (long)gridDim.x * kBlock;
    unsigned acc = 0;
    const long N4 = N / 4;
    for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < N4; i += stride) {
        PfAugRgb c[4];
        pf_aug_load4(src + i * 12, c);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc += (unsigned)pf_aug_luma(pf_aug_chain(c[j], s, 0, upto));
    }
    if (blockIdx.x == 0 && threadIdx.x < (int)(N - N4 * 4))
        acc += (unsigned)pf_aug_luma(pf_aug_chain(pf_aug_load(src + (N4 * 4 + threadIdx.x) * 3), s, 0, upto));
    const unsigned long long t = pf_aug_block_sum(acc, red);
    if (threadIdx.x == 0) atomicAdd(a.sums + (long)b * PF_AUG_SUMS + second, t);
}

struct PfAugImg { PfAugSet s; int mean; int r; };
__device__ __forceinline__ PfAugImg pf_aug_image_setup(const PfAugArgs& a, const int* row, int b, int img) {
    PfAugImg m;
    const int second = pf_aug_second(row, img);
    m.s = pf_aug_set(row, second);
    const unsigned long long n = (unsigned long long)a.H * a.W * ((row[PF_AUG_MODE] & PF_AUG_ASYM_COLOUR) ? 1 : 2);
    m.mean = pf_aug_mean(a.sums[(long)b * PF_AUG_SUMS + second], n);
    m.r = pf_aug_wrap(row[img ? PF_AUG_R2 : PF_AUG_R1], a.W);
    return m;
}

// grid (blocks, 3, B): y = 0, 1 the images, 2 the flow.  VEC: a thread owns four consecutive output pixels of a row (16-byte
// stores per plane) and gathers its sources from (x - r) mod W; otherwise one output pixel per thread.  The same per-pixel
// functions either way.
template <bool VEC>
__global__ void __launch_bounds__(kBlock) pf_aug_main_kernel(const PfAugArgs a) {
    __shared__ unsigned long long red[4];
    constexpr int PX = VEC ? 4 : 1;
    const int b = blockIdx.z, what = blockIdx.y, W = a.W;
    const int* row = a.params + (long)b * PF_AUG_ROW;
    const long N = (long)a.H * W, items = N / PX;
    const long stride = (long)gridDim.x * kBlock;
    if (what == 2) {
        const int asym = (row[PF_AUG_MODE] & PF_AUG_ASYM_ROLL) ? 1 : 0;
        const int r1 = row[PF_AUG_R1], r2 = row[PF_AUG_R2], r = pf_aug_wrap(r1, W);
        const float* f = a.flow + (long)b * N * 2;
        float* ou = a.oflow + (long)b * 2 * N;
        float* ov = a.ovalid + (long)b * N;
        for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < items; i += stride) {
            const long n = i * PX;
            const int y = (int)(n / W), x = (int)(n - (long)y * W);
            PfAugFlow o[4];
#pragma unroll
            for (int j = 0; j < PX; ++j) {
                int xs = x + j - r;
                if (xs < 0) xs += W;
                const float* p = f + ((long)y * W + xs) * 2;
                o[j] = pf_aug_flow(p[0], p[1], W, asym, r1, r2);
            }
            if (VEC) {
                *reinterpret_cast<float4*>(ou + n) = make_float4(o[0].u, o[1].u, o[2].u, o[3].u);
                *reinterpret_cast<float4*>(ou + N + n) = make_float4(o[0].v, o[1].v, o[2].v, o[3].v);
                *reinterpret_cast<float4*>(ov + n) = make_float4(o[0].valid, o[1].valid, o[2].valid, o[3].valid);
            } else {
                ou[n] = o[0].u; ou[N + n] = o[0].v; ov[n] = o[0].valid;
            }
        }
        return;
    }
    const PfAugImg m = pf_aug_image_setup(a, row, b, what);
    const unsigned char* src = a.img[what] + (long)b * N * 3;
    float* out = a.out[what] + (long)b * 3 * N;
    unsigned sr = 0, sg = 0, sb = 0;
    for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < items; i += stride) {
        const long n = i * PX;
        const int y = (int)(n / W), x = (int)(n - (long)y * W);
        int xs = x - m.r;
        if (xs < 0) xs += W;
        PfAugRgb c[4];
        if (VEC) {
            if (xs + 3 < W) {
                pf_aug_load4(src + ((long)y * W + xs) * 3, c);
            } else {                                        // the seam: each pixel wraps on its own
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int xj = xs + j < W ? xs + j : xs + j - W;
                    c[j] = pf_aug_load(src + ((long)y * W + xj) * 3);
                }
            }
        } else {
            c[0] = pf_aug_load(src + ((long)y * W + xs) * 3);
        }
#pragma unroll
        for (int j = 0; j < PX; ++j) {
            c[j] = pf_aug_chain(c[j], m.s, m.mean, 4);
            sr += (unsigned)c[j].r; sg += (unsigned)c[j].g; sb += (unsigned)c[j].b;
        }
        if (VEC) {
            *reinterpret_cast<float4*>(out + n) = make_float4((float)c[0].r, (float)c[1].r, (float)c[2].r, (float)c[3].r);
            *reinterpret_cast<float4*>(out + N + n) = make_float4((float)c[0].g, (float)c[1].g, (float)c[2].g, (float)c[3].g);
            *reinterpret_cast<float4*>(out + 2 * N + n) = make_float4((float)c[0].b, (float)c[1].b, (float)c[2].b, (float)c[3].b);
        } else {
            out[n] = (float)c[0].r; out[N + n] = (float)c[0].g; out[2 * N + n] = (float)c[0].b;
        }
    }
    if (what == 1 && row[PF_AUG_NRECT] > 0) {               // the eraser's mean colour: image 2 after the colour step
        const unsigned long long tr = pf_aug_block_sum(sr, red), tg = pf_aug_block_sum(sg, red), tb = pf_aug_block_sum(sb, red);
        if (threadIdx.x == 0) {
            unsigned long long* s = a.sums + (long)b * PF_AUG_SUMS + 2;
            atomicAdd(s, tr); atomicAdd(s + 1, tg); atomicAdd(s + 2, tb);
        }
    }
}

// grid (blocks, 2 rectangles, B): image 2 only, both rectangles with the one mean (augmentor.py:245-251); the rectangle was
// clipped before the roll, so it may straddle the seam afterwards
__global__ void __launch_bounds__(kBlock) pf_aug_erase_kernel(const PfAugArgs a) {
    const int b = blockIdx.z;
    const int* row = a.params + (long)b * PF_AUG_ROW;
    int x0, y0, w, h;
    if (!pf_aug_rect(row, blockIdx.y, a.H, a.W, x0, y0, w, h)) return;
    const long N = (long)a.H * a.W;
    const unsigned long long* s = a.sums + (long)b * PF_AUG_SUMS + 2;
    const float mr = (float)(s[0] / (unsigned long long)N), mg = (float)(s[1] / (unsigned long long)N),
                mb = (float)(s[2] / (unsigned long long)N);
    const int r = pf_aug_wrap(row[PF_AUG_R2], a.W);
    float* out = a.out[1] + (long)b * 3 * N;
    const int total = w * h;
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < total; i += gridDim.x * kBlock) {
        const int yy = y0 + i / w;
        int xx = x0 + i % w + r;
        if (xx >= a.W) xx -= a.W;
        const long n = (long)yy * a.W + xx;
        out[n] = mr; out[N + n] = mg; out[2 * N + n] = mb;
    }
}

// 8-bit colour conversion of n pixels: mode 0 RGB -> HSV, 1 HSV -> RGB (Pillow's Image.convert)
__global__ void __launch_bounds__(kBlock) pf_aug_convert_kernel(const unsigned char* in, unsigned char* out, long n, int mode) {
    const long stride = (long)gridDim.x * kBlock;
    for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const PfAugRgb c = pf_aug_load(in + i * 3);
        const PfAugRgb o = mode ? pf_aug_hsv_to_rgb(c.r, c.g, c.b) : pf_aug_rgb_to_hsv(c);
        out[i * 3] = (unsigned char)o.r; out[i * 3 + 1] = (unsigned char)o.g; out[i * 3 + 2] = (unsigned char)o.b;
    }
}

unsigned pf_aug_blocks(long items) {
    long blocks = (items + kBlock - 1) / kBlock;
    return (unsigned)(blocks < 1 ? 1 : (blocks > kMaxBlocks ? kMaxBlocks : blocks));
}
}  // namespace

extern "C" long pf_augment_scratch_bytes(int B) { return pf_augment_scratch_bytes_impl(B); }

extern "C" int pf_augment_360(const unsigned char* img1, const unsigned char* img2, const float* flow, const int* params,
                              float* image1, float* image2, float* flow_gt, float* valid, void* scratch, long scratch_bytes,
                              int B, int H, int W, void* stream) {
    const int rc = pf_augment_check(img1, img2, flow, params, image1, image2, flow_gt, valid, scratch, scratch_bytes, B, H, W);
    if (rc != PF_OK) return rc;
    PfAugArgs a;
    a.img[0] = img1; a.img[1] = img2; a.flow = flow; a.params = params;
    a.out[0] = image1; a.out[1] = image2; a.oflow = flow_gt; a.ovalid = valid;
    a.sums = reinterpret_cast<unsigned long long*>(scratch);
    a.B = B; a.H = H; a.W = W;
    hipStream_t st = (hipStream_t)stream;
    const long N = (long)H * W;
    hipLaunchKernelGGL(pf_aug_zero_kernel, dim3((unsigned)((B * PF_AUG_SUMS + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, a.sums,
                       B * PF_AUG_SUMS);
    hipLaunchKernelGGL(pf_aug_contrast_kernel, dim3(pf_aug_blocks(N / 4), 2, (unsigned)B), dim3(kBlock), 0, st, a);
    const bool vec = W % 4 == 0 &&
                     ((uintptr_t)image1 | (uintptr_t)image2 | (uintptr_t)flow_gt | (uintptr_t)valid) % 16 == 0;
    if (vec)
        hipLaunchKernelGGL(pf_aug_main_kernel<true>, dim3(pf_aug_blocks(N / 4), 3, (unsigned)B), dim3(kBlock), 0, st, a);
    else
        hipLaunchKernelGGL(pf_aug_main_kernel<false>, dim3(pf_aug_blocks(N), 3, (unsigned)B), dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(pf_aug_erase_kernel, dim3(40, 2, (unsigned)B), dim3(kBlock), 0, st, a);
    return (int)hipGetLastError();
}

extern "C" int pf_augment_convert(const unsigned char* in, unsigned char* out, long n, int mode, void* stream) {
    if (!in || !out || in == out || (mode != 0 && mode != 1)) return PF_ERR_BAD_ARG;
    if (n < 1 || n >= (1L << 30)) return PF_ERR_BAD_SHAPE;
    hipLaunchKernelGGL(pf_aug_convert_kernel, dim3(pf_aug_blocks(n)), dim3(kBlock), 0, (hipStream_t)stream, in, out, n, mode);
    return (int)hipGetLastError();
}
