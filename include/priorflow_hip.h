/* priorflow_hip.h -- C-ABI of the MI355X-native PriOr-RAFT inner loop (libpriorflow_hip.so).
 *
 * The reference (longliangLiu/PriOr-Flow, directory PriOr-RAFT/) has no FFI / plugin
 * boundary of its own: its hot path is a chain of Python functions calling torch ops.
 * Each entry point below replaces one of those functions (cited file:line, relative to
 * PriOr-RAFT/) with a hand-written gfx950 kernel.  INTEGRATION.md shows the ctypes
 * binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every function returns 0 on success, a positive hipError_t on a HIP failure, or a
 *     negative PF_ERR_* code on a bad argument; nothing throws, allocates or frees;
 *   - all buffers are DEVICE pointers owned by the caller, fp32, 16-byte aligned;
 *   - work is enqueued on `stream` (a hipStream_t passed as void*) without synchronising;
 *   - "planar" = [B,2,H8*W8] (NCHW with 2 channels); "channel-last" = [B*H8*W8][ld] with the
 *     logical channels at columns [c_off, c_off+C) of each row (lets producers write straight
 *     into slices of a wider concatenation buffer: torch.cat never materialises);
 *   - n = y*W8 + x is the raster index of a 1/8-resolution pixel, N = H8*W8;
 *   - sample grids are [2,H,W] (m', n') and shared by every batch element.
 */
#ifndef PRIORFLOW_HIP_H
#define PRIORFLOW_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define PF_OK 0
#define PF_ERR_BAD_ARG (-1)
#define PF_ERR_BAD_SHAPE (-2)

/* Library / build identification ("gfx950 fp32-mfma ..."). */
const char* pf_version(void);

/* ---- ERP geometry ---------------------------------------------------------------------- */

/* generate_samplegrid (core/utils/projection_prim_ortho.py:432-443): ERP pixel -> sphere ->
 * R -> ERP pixel.  R is 9 HOST floats, row-major.  grid: [2,H,W]. */
int pf_sample_grid(float* grid, int H, int W, const float* R_host, void* stream);

/* img_rotate (core/utils/projection_prim_ortho.py:507-514): wrap-x / zero-pad bilinear resample
 * of an NCHW image stack with a sample grid.  img,out: [B,C,H,W]. */
int pf_img_rotate(const float* img, const float* grid, float* out, int B, int C, int H, int W,
                  void* stream);

/* Input normalisation `2 * (image / 255.0) - 1.0` of both images (core/prior_raft.py:121-122; IEEE division, as the
 * reference's CPU path), written straight into the encoders' batches: image1 -> f1 and (optional) c1, image2 -> f2.
 * count = B*3*H*W elements per image. */
int pf_normalise_images(const float* image1, const float* image2, float* f1, float* f2, float* c1,
                        long count, void* stream);

/* The input stage of a forward in one launch (core/prior_raft.py:121-127): both images normalised as pf_normalise_images does and
 * resampled into view B as pf_img_rotate does with `grid` ([2,H,W], generate_samplegrid of R_A2B), written into the encoders'
 * batches img_f = [im1 | im2 | im1_B | im2_B] ([4B,3,H,W]) and, optionally, img_c = [im1 | im1_B] ([2B,3,H,W]; NULL to skip).
 * Bit-identical to pf_normalise_images + pf_img_rotate on the normalised pair.  image1, image2: [B,3,H,W], values 0..255. */
int pf_prepare_images(const float* image1, const float* image2, const float* grid, float* img_f, float* img_c,
                      int B, int H, int W, void* stream);

/* The input stage of ONE frame (video streams): out = [im | im_B] ([2B,3,H,W]), bit-identical to img_c of pf_prepare_images with
 * image1 = image.  image: [B,3,H,W], values 0..255; grid as in pf_prepare_images. */
int pf_prepare_frame(const float* image, const float* grid, float* out, int B, int H, int W, void* stream);

/* forward_interpolate (core/utils/utils.py:30-58): the warm start of a flow sequence, batched.  flow, out: planar [B,2,h,w].
 * Source pixel (x0, y0) moves to (x1, y1) = (x0 + u, y0 + v) (float64); it is a valid point iff 0 < x1 < w and 0 < y1 < h
 * (strict).  Every pixel of out takes the (u, v) of the valid point nearest to it (Euclidean, float64; equally near: the lowest
 * source raster index); an image without a valid point gives zeros.  wrap = 1 (ERP): x1 is taken modulo w, the x test always
 * holds, and x distances wrap, min(|dx|, w - |dx|).  Exact: a counting sort of the points into unit cells and a ring search
 * per pixel (five launches, no host synchronisation).  scratch: device memory of at least 4 * B * (3 * h * w + 1) bytes,
 * overwritten.  PF_ERR_BAD_ARG: a NULL pointer, flow == out, wrap not 0 / 1 or scratch_bytes too small. */
int pf_forward_interpolate(const float* flow, float* out, void* scratch, long scratch_bytes, int B, int h, int w, int wrap,
                           void* stream);

/* Forward-backward consistency of two opposite ERP flow fields, both directions in ONE launch (no host synchronisation).
 * flow_fw (frame 0 -> 1, on frame 0's grid) and flow_bw (frame 1 -> 0, on frame 1's grid): NCHW [B,2,H,W], pixels.
 * For a direction with flow f and opposite flow g, at pixel p = (x, y):
 *   q = p + f;  g^ = g sampled at q with the model's cyclic sampler (x wrapped, y clamped, weights from the unclamped
 *   fraction: core/utils/my_cycle_sample.py:31-60), the u component of the three non-anchor taps first brought to within W/2
 *   of the anchor tap (as flo_rotate's seam handling, :82-97), v blended plainly;
 *   round trip r = (u_clip(f_u + g^_u), f_v + g^_v), u_clip(t) = pymod(t + W/2, W) - W/2;
 *   PF_FB_PLANE:  occluded <=> |r|^2 > alpha (|f|^2 + |g^|^2) + beta;
 *   PF_FB_SPHERE: with d(a, b) the Haversine great-circle distance (R = 1) of two ERP points under the pixel -> (theta, phi)
 *     map of pf_flow_metrics, y NOT clamped and the haversine clamped to [0, 1] (a point past a pole never gives NaN):
 *     s_r = d(p, p + r), s_f = d(p, q), s_g = d(q, p + r);  occluded <=> s_r^2 > alpha (s_f^2 + s_g^2) + beta (2 pi / W)^2
 *     (beta keeps its meaning of squared pixels at the equator).
 *   A non-finite f or g^ gives occluded = 1 and r = 0.
 * occ_fw / occ_bw: [B,H,W] bytes (1 = the round trip fails); res_fw / res_bw: [B,2,H,W] fp32 (r, pixels).
 * PF_ERR_BAD_ARG: a NULL pointer, an output aliasing an input or another output, metric not PF_FB_*, alpha or beta negative
 * or not finite.  PF_ERR_BAD_SHAPE: B < 1, H or W < 2, or H * W >= 2^30. */
#define PF_FB_PLANE 0
#define PF_FB_SPHERE 1
int pf_fb_check(const float* flow_fw, const float* flow_bw, unsigned char* occ_fw, unsigned char* occ_bw, float* res_fw,
                float* res_bw, int B, int H, int W, int metric, float alpha, float beta, void* stream);

/* Chained ERP flows: long-range flow and point tracks.  One statement, for a point p = (px, py) in pixels
 * with px UNWRAPPED (any real number: longitude winds), a flow g [2,H,W] and optionally a mask occ_g [H,W] of bytes (any
 * non-zero byte counts as 1):
 *   g^(p) = g sampled at p with the model's cyclic sampler exactly as pf_fb_check samples: x wrapped with the Python modulo,
 *     y clamped, the bilinear weights from the unclamped fraction, the u component of the three non-anchor taps first brought
 *     to within W/2 of the anchor tap, v blended plainly;
 *   m(p) = sum w_i occ_i over the same four taps and weights (0 when occ_g is NULL);
 *   p' = p + g^(p).  u is NOT clipped to +-W/2: accumulated displacement keeps its winding, only the sampler wraps.
 *   State is one byte per point and sticky: state' = state | new bits,
 *     PF_TRK_OCCLUDED   m(p) >= 0.5;
 *     PF_TRK_POLE       py < -0.5 or py > H - 0.5: the point has left the map through a pole (the sampler still clamps);
 *     PF_TRK_NONFINITE  the position or a sampled value is not finite; the displacement added is then 0.
 *   A point with state != 0 is still advanced (dead reckoning); callers mask by state.
 *
 * pf_flow_compose, the dense form: out(x) = f(x) + g^(x + f(x)) on the pixel grid, state_out(x) = state_f(x) | new bits, for
 * njobs = 1..PF_COMPOSE_MAX jobs of one geometry in ONE launch (jobs: host memory, copied into the kernel arguments).  f, g,
 * out: NCHW [B,2,H,W]; state_f (NULL: read as 0), occ_g (NULL: no mask), state_out (NULL: not written): [B,H,W] bytes.  out may
 * be f and state_out may be state_f (each pixel is read before it is written).  The jobs of a launch run unordered.
 * PF_ERR_BAD_ARG: njobs outside 1..PF_COMPOSE_MAX, a NULL jobs / f / g / out, out == g, state_out == occ_g, or an output of one
 * job that is an operand or output of another.  PF_ERR_BAD_SHAPE: B, H or W < 1, or H * W >= 2^30.  Every refusal answers before
 * anything is launched.  No scratch memory, no atomics, capturable.
 *
 * pf_track_points, the sparse form, in place: pos [B,N,2] fp32 (x, y) with x unwrapped, state [B,N] bytes, flow [B,2,H,W], occ
 * [B,H,W] bytes or NULL:  pos <- pos + g^(pos), state <- state | new bits.  PF_ERR_BAD_ARG: a NULL pos / state / flow.
 * PF_ERR_BAD_SHAPE: B, N, H or W < 1, or H * W >= 2^30.
 * pf_track_grid writes the pixel centres (x, y) of an H x W map as pos [B,H*W,2]: one step of a tracker started there equals
 * the grid plus pf_flow_compose of a zero flow, bit for bit. */
#define PF_TRK_OCCLUDED 1
#define PF_TRK_POLE 2
#define PF_TRK_NONFINITE 4
#define PF_COMPOSE_MAX 4
typedef struct pf_compose_job {
    const float* f; const unsigned char* state_f;
    const float* g; const unsigned char* occ_g;
    float* out; unsigned char* state_out;
} pf_compose_job;
int pf_flow_compose(const pf_compose_job* jobs, int njobs, int B, int H, int W, void* stream);
int pf_track_points(float* pos, unsigned char* state, const float* flow, const unsigned char* occ, int B, int N, int H, int W,
                    void* stream);
int pf_track_grid(float* pos, int B, int H, int W, void* stream);

/* Order statistic on the device: out[b] = np.sort(x[b])[k] for each image of x [B, n] (fp32, NON-NEGATIVE values: a length),
 * 0 <= k < n, bit for bit, equal values included; no host read, no allocation, capturable.  A radix select over the bit pattern
 * (11 + 11 + 10 bits; LDS histograms, one integer atomic per non-empty bin and workgroup, so the result does not depend on the
 * order of the adds): five launches.  +inf is an ordinary largest value.  NaN ranks last, as numpy sorts it; when rank k falls on
 * a NaN the result is the largest value that is not NaN (0 when there is none).  Outside the contract: a value with the sign bit
 * set counts as +0.  scratch: device memory of at least pf_order_stat_scratch_bytes(B, n) bytes, 4-byte aligned, overwritten.
 * PF_ERR_BAD_ARG: a NULL pointer, x == out, k outside [0, n) or scratch_bytes too small.  PF_ERR_BAD_SHAPE: B < 1,
 * B > PF_MAX_IMAGES (an image is one row of the launch grid), n < 1, n >= 2^31. */
#define PF_MAX_IMAGES 65535
long pf_order_stat_scratch_bytes(int B, long n);
int pf_order_stat(const float* x, float* out, void* scratch, long scratch_bytes, int B, long n, long k, void* stream);

/* Colour coding of flow fields (core/utils/flow_viz.py): flow NCHW [B,2,H,W] fp32 -> 8-bit image, per image of the batch.
 *   PF_RENDER_OMNI  = omniflow_to_image (:144-215, clip_flow = None): len = great-circle length of the flow
 *                     (calculate_veclen_spherical, core/utils/spherical.py:56-70; R = 1), clip = sort(len)[k],
 *                     k = min(int(percentile * H * W), H * W - 1) computed in double (the reference: 0.95);
 *   PF_RENDER_PLANE = flow_to_image (:117-141): len = |flow|, clip = max len (percentile ignored).
 *   rad = min(len, clip) / (clip + 1e-5); a = atan2(-v, -u) / pi; fk = (a + 1) / 2 * 54 blends entries floor(fk) and floor(fk) + 1
 *   (55 -> 0) of the 55-entry Middlebury wheel; col = 1 - rad (1 - blend) (rad > 1: 0.75 blend); byte = floor(255 col); all fp32.
 * A pixel whose flow is not finite counts as NaN in the order statistic (pf_order_stat: it ranks last) and is written (0, 0, 0);
 * every finite flow has a finite length (the haversine is clamped to 1: an antipodal end point never gives NaN) and is ranked.
 * out: PF_LAYOUT_HWC [B,H,W,3] or PF_LAYOUT_CHW [B,3,H,W]; bgr = 1 reverses the channel order (convert_to_bgr).
 * Five launches, no host read: zero the counts; len to scratch fused with the first select pass; two select passes; colourise
 * (each workgroup makes the last choice of the select itself).  Four pixels of a row per thread when W % 4 == 0, flow and scratch
 * are 16-byte aligned and out 4-byte aligned, one pixel per thread otherwise: the same per-pixel function, the same bytes.
 * scratch: at least pf_flow_render_scratch_bytes(B, H, W) bytes, overwritten; afterwards it starts with len [B,H,W] fp32, followed
 * by clip [B] fp32.  PF_ERR_BAD_ARG: a NULL pointer, flow == out, mode / layout / bgr not one of their values, percentile outside
 * [0, 1] or scratch_bytes too small.  PF_ERR_BAD_SHAPE: B < 1, B > PF_MAX_IMAGES, H or W < 2, H * W >= 2^30. */
#define PF_RENDER_OMNI 0
#define PF_RENDER_PLANE 1
#define PF_LAYOUT_HWC 0
#define PF_LAYOUT_CHW 1
long pf_flow_render_scratch_bytes(int B, int H, int W);
int pf_flow_render(const float* flow, unsigned char* out, void* scratch, long scratch_bytes, int B, int H, int W, int mode,
                   double percentile, int layout, int bgr, void* stream);

/* my_cycle_warp (core/utils/my_cycle_sample.py:100-115): out[b,c,y,x] = x[b,c] sampled at (x + u, y + v), (u, v) = flo[b,:,y,x],
 * with the model's cyclic sampler (x wrapped, y clamped, weights from the unclamped fraction; no seam un-wrapping).  x, out:
 * [B,C,H,W] fp32, any C >= 1; flo: [B,2,H,W].  The taps of a pixel are computed once for its C channels.  ref (frame 1, [B,C,H,W])
 * and err ([B,H,W]) are given together or both NULL: err = mean over c of |ref - out|, written by the same launch.  A flow that is
 * not finite gives NaN in out (and err) at that pixel; every read stays inside the maps.
 * PF_ERR_BAD_ARG: a NULL x / flo / out, an output aliasing an input or the other output, only one of ref / err.
 * PF_ERR_BAD_SHAPE: B or C < 1, H or W < 2, H * W >= 2^30. */
int pf_cycle_warp(const float* x, const float* flo, const float* ref, float* out, float* err, int B, int C, int H, int W,
                  void* stream);

/* Training augmentation for the 360-degree sets: what FlowDataset_360.__getitem__ with
 * FlowAugmentor_360(do_flip=False) delivers (core/datasets.py:137-159, core/utils/augmentor.py:210-316), for B samples at once.
 *   img1, img2: [B,H,W,3] bytes as decoded; flow: [B,H,W,2] fp32 as decoded; params: [B][PF_AUG_ROW] 32-bit words, one row
 *   per sample (the layout: csrc/pf_augment.h, mirrored by prior_flow_amd.augment.AugmentParams), already on the device.
 *   image1, image2: [B,3,H,W] fp32 (integer values 0..255); flow_gt: [B,2,H,W]; valid: [B,H,W] (0 / 1), fp32.
 * Per sample, in the reference's order: u = (u + W/2) % W - W/2 (datasets.py:138); the colour step (augmentor.py:228-239: one
 * ColorJitter draw on the stack of both images, or one per image when the row's asymmetric bit is set; torchvision's PIL
 * backend: 8 bits after every operation, Image.blend in fp32 with truncation, Pillow's L and HSV; the contrast mean
 * int(mean(L) + 0.5) is taken over what the draw is applied to); the eraser (:241-252: up to two rectangles clipped at the border,
 * filled in image 2 with its truncated per-channel mean after the colour step); the yaw roll (:254-283: out[:, (m + r) % W] =
 * in[:, m]; image 1 and the flow by r1, image 2 by r2, and u = u_clip((u + r2) - r1) when the row's asymmetric-roll bit is
 * set); valid = |u| < 1000 & |v| < 1000 (datasets.py:158; NaN gives 0).
 * Four launches on `stream`, no host read, no allocation, capturable: zero the sums; the L sums for the contrast means; the
 * main pass (chain, roll, flow, valid, image 2's channel sums); the eraser.  All sums are 64-bit integers (one atomic per
 * workgroup and quantity), so repeated launches are identical.  Four output pixels of a row per thread when W % 4 == 0 and the
 * four outputs are 16-byte aligned, one pixel per thread otherwise: the same per-pixel functions, the same bytes.
 * A row's values are not trusted: rolls are reduced mod W, rectangles clipped, unknown operations skipped.
 * scratch: at least pf_augment_scratch_bytes(B) bytes, 8-byte aligned, overwritten.
 * PF_ERR_BAD_ARG: a NULL pointer, two outputs that are the same, a misaligned scratch / params / flow, scratch_bytes too small.
 * PF_ERR_BAD_SHAPE: B < 1, B > PF_MAX_IMAGES, H or W < 2, H * W >= 2^30. */
#define PF_AUG_ROW_WORDS 32
long pf_augment_scratch_bytes(int B);
int pf_augment_360(const unsigned char* img1, const unsigned char* img2, const float* flow, const int* params, float* image1,
                   float* image2, float* flow_gt, float* valid, void* scratch, long scratch_bytes, int B, int H, int W,
                   void* stream);
/* Pillow's 8-bit Image.convert between RGB and HSV on n interleaved pixels: mode 0 RGB -> HSV, 1 HSV -> RGB.  The two halves of
 * the hue step of pf_augment_360, callable on their own: a parameter row can only run the round trip, and HSV -> RGB alone is
 * held to Pillow bit for bit on the device as well.  PF_ERR_BAD_ARG: NULL, in == out, another mode; PF_ERR_BAD_SHAPE: n < 1 or
 * n >= 2^30. */
int pf_augment_convert(const unsigned char* in, unsigned char* out, long n, int mode, void* stream);

/* out[b] = mean of x[b, :] over the elements with mask[b, n] == 0 (mask NULL: all of them; nothing counted: 0).  x: [B,N] fp32,
 * mask: [B,N] bytes.  fp64 sums of at most 64 chunks per image, then one sum in chunk order: deterministic, two launches, no
 * host read.  scratch: at least 1024 * B bytes, 8-byte aligned.  PF_ERR_BAD_ARG: a NULL x / out / scratch, out == x, scratch
 * misaligned or too small.  PF_ERR_BAD_SHAPE: B < 1, B > PF_MAX_IMAGES, N < 1, N >= 2^30. */
int pf_masked_mean(const float* x, const unsigned char* mask, float* out, void* scratch, long scratch_bytes, int B, int N,
                   void* stream);

/* Perspective viewports and cube maps of ERP frames and ERP flow.  Geometry, the reference's convention
 * (core/utils/projection_prim_ortho.py:264-430; its diverge_zero nudge is not applied):
 *   ERP pixel (m, n): theta = ((m + 1/2) / W - 1/2) 2 pi, phi = (1/2 - (n + 1/2) / H) pi, s(m, n) = (cos phi cos theta,
 *   cos phi sin theta, sin phi); a direction d lies at theta = atan2(d_y, d_x), phi = asin(d_z / |d|),
 *   m = (theta / 2 pi + 1/2) W - 1/2, n = (1/2 - phi / pi) H - 1/2.
 *   A view is (R, f, h, w): R 3x3 with columns forward, right, up in world axes, f the focal length in pixels, principal point
 *   (c_x, c_y) = ((w - 1) / 2, (h - 1) / 2).  Pixel (i, j) has the camera ray (1, (j - c_x) / f, -(i - c_y) / f) and the world
 *   ray d = R ray; proj(q) = (c_x + f q_r / q_f, c_y - f q_u / q_f), (q_f, q_r, q_u) = R^T q.  With R = I the view looks at the
 *   ERP centre, right is +m and down is +n.
 * views_host: V rows of PF_VIEW_WORDS HOST floats {R row-major, f, h, w}, 1 <= V <= PF_VIEW_MAX, every row with the same h x w;
 * the table travels to the kernel as an argument (no copy to the device, the call can be captured; a captured call keeps the
 * table it was captured with).  One thread per output pixel; ray, position and taps are computed once for all channels.
 * Every entry: one launch, no host read, no allocation.  PF_ERR_BAD_ARG: a NULL pointer, an output aliasing an input or the other
 * output, an R entry or f that is not finite, f <= 0, an unknown form, min_forward outside (0, 1).  PF_ERR_BAD_SHAPE: V outside
 * 1..PF_VIEW_MAX, h or w that is no integer in 1..32768 or differs between rows, B, C, H, W or s < 1, C > 4096, H * W or
 * h * w >= 2^30, B * V > 65535 (an image of a view is one row of the launch grid).
 *
 * pf_viewport_image: ERP -> views, sampled at the ray's (m, n) with the model's cyclic taps (x wraps, y clamps, weights from the
 *   unclamped fraction: rays towards a pole read the pole row).  PF_VIEW_F32: in [B,C,H,W] fp32 -> out [B,V,C,h,w] fp32;
 *   PF_VIEW_U8: in [B,H,W,C] bytes (what pf_flow_render writes) -> out [B,V,h,w,C] bytes, floor(x + 1/2) clamped to 0..255.
 *   No anti-aliasing: a view coarser than the panorama is point-sampled with four taps.
 * pf_viewport_flow: ERP flow [B,2,H,W] -> pinhole flow out [B,V,2,h,w] (view pixels; channel 0 along j, 1 along i) and valid
 *   [B,V,h,w] bytes.  For the pixel's unit ray p^ and the four taps k (weights w_k) of its position: s_k = s(m_k, n_k),
 *   e_k = s(m_k + u_k, clamp(n_k + v_k, -1/2, H - 1/2)) (flow2endpoint's rule), q = p^ + sum w_k (e_k - s_k),
 *   out = proj(q) - proj(p^).  The 3-D displacement is interpolated, never u or v: the seam needs no un-wrapping, a zero flow
 *   gives exactly (0, 0), and the result is second-order accurate in the pixel pitch.  valid = 1 exactly when the flows of all
 *   four taps are finite and q_f > min_forward |q| (the default of the Python layer: cos 85 deg); where valid = 0 out is (0, 0).
 *   Every read stays inside the maps for any input bits.
 * pf_cubemap_to_erp: faces [B,6,C,s,s] fp32 -> out [B,C,H,W].  Faces in the order front, right, back, left, up, down with R columns
 *   [forward, right, up] = [+x +y +z], [+y -x +z], [-x -y +z], [-y +x +z], [+z +y -x], [-z +y +x] and f = s / 2.  Per ERP pixel
 *   d = s(m, n); the face is the axis with the largest |component| (ties: the earlier face); bilinear at proj(d) with the taps
 *   clamped to that face.  No filtering across face edges. */
#define PF_VIEW_MAX 16
#define PF_VIEW_WORDS 12
#define PF_VIEW_F32 0
#define PF_VIEW_U8 1
int pf_viewport_image(const void* in, void* out, const float* views_host, int V, int B, int C, int H, int W, int form,
                      void* stream);
int pf_viewport_flow(const float* flow, const float* views_host, int V, float* out, unsigned char* valid, int B, int H, int W,
                     float min_forward, void* stream);
int pf_cubemap_to_erp(const float* faces, float* out, int B, int C, int s, int H, int W, void* stream);

/* Forward softmax splatting (the statement is prior-flow_amd/csrc/pf_splat.h): maps are moved ALONG their
 * flow and blended, e.g. the frame at time t between two frames from the two flows between them.  Two launches per call:
 *
 * pf_splat_accumulate: njobs = 1..PF_SPLAT_MAX jobs of one geometry (jobs: host memory, copied into the kernel arguments).  Job j:
 *   src [B,C,H,W] fp32 (C = 1..4), flow [B,2,H,W], metric [B,cm,H,W] or NULL (cm = 1: m = |metric|, cm = 2: the Euclidean length
 *   of the two planes), mask [B,H,W] bytes or NULL (non-zero: the pixel is skipped), tau (how far along the flow), beta in (0, 1].
 *   Source pixel (x, y): q = (x + tau u, y + tau v) in fp32; w = beta expf(-min(alpha m, zmax)) (beta without a metric or at
 *   alpha = 0); skipped when masked or when q, m or one of its values is not finite (|q| >= 2^30 counts as not finite); four
 *   bilinear taps, the columns wrapped with the Python modulo, a row outside [0, H - 1] dropped (not clamped); per target p
 *     N_c[p] += w b_k clamp(src_c, +-vmax),  D[p] += w b_k,  cov[p] += beta b_k
 *   as 64-bit INTEGERS: each contribution is llrintf(value * 2^S) with S_D = S_cov = 62 - ceil(log2(njobs H W)) and
 *   S_N = S_D - ceil(log2(vmax)), so no sum can overflow and the result does not depend on the order of the adds.
 *   acc: [B][C+2][H][W] int64 (pf_splat_scratch_bytes), all-zero on entry.
 * pf_splat_resolve: per target pixel hole = cov < cmin (or D <= 0), out_c = N_c / D; a hole takes (1 - fill_t) fill0 + fill_t
 *   fill1 ([B,C,H,W] maps, both or neither) or 0; hole [B,H,W] bytes; the sums are written back as zeros: acc is all-zero again.
 *   njobs and vmax must be the accumulate call's (they fix the scales).
 * PF_ERR_BAD_ARG: a NULL jobs / acc / src / flow / out / hole, njobs outside 1..PF_SPLAT_MAX, C outside 1..4, cm outside {1, 2}
 * with a metric, tau not finite, beta outside (0, 1], alpha < 0, zmax < 0, vmax outside [1, 65536], cmin <= 0, acc not 8-byte
 * aligned or aliasing an operand, one fill map without the other, fill_t outside [0, 1], out aliasing a fill map (a source).
 * PF_ERR_BAD_SHAPE: B, H or W < 1, B > 65535, H * W >= 2^30.  Every refusal answers before anything is launched.  No host read,
 * no allocation, capturable. */
#define PF_SPLAT_MAX 4
typedef struct pf_splat_job {
    const float* src; const float* flow;
    const float* metric; const unsigned char* mask;
    int cm; float tau; float beta;
} pf_splat_job;
long pf_splat_scratch_bytes(int B, int C, int H, int W);
int pf_splat_accumulate(const pf_splat_job* jobs, int njobs, void* acc, int B, int C, int H, int W, float alpha, float zmax,
                        float vmax, void* stream);
int pf_splat_resolve(void* acc, float* out, unsigned char* hole, const float* fill0, const float* fill1, float fill_t, float cmin,
                     int njobs, int B, int C, int H, int W, float vmax, void* stream);

/* Camera rotation from 360-degree flow, and stabilisation (the statement is
 * prior-flow_amd/csrc/pf_egomotion.h).  On the sphere a camera rotation moves every bearing rigidly: with p = s(x, y) and
 * q = s(x + u, clamp(y + v, -1/2, H - 1/2)) (the ERP convention of the viewports above) the rotation sought has q ~ R p.  A pixel
 * is left out when its mask byte is non-zero or |u| or |v| is not below 2^30 (not finite included).  Every matrix is nine fp32
 * values row-major in DEVICE memory, [B,9].
 *
 * pf_ego_accumulate: one pass over flow [B,2,H,W] (mask [B,H,W] bytes or NULL): the twelve sums per image S_ab = sum w p_a q_b,
 *   sum w, sum w r^2 and the number of pixels used, added into sums [B,12] int64 (pf_ego_scratch_bytes; all-zero before the
 *   first pass).  w = cos phi(y) without weights (weighted = 0), times the Geman-McClure weight 1 / (1 + r^2 / c^2)^2 with
 *   weighted = 1; r = |q - R p| is the chord under the matrix R of the pass before, c = scale_px 2 pi / W.  The sums are INTEGERS, a
 *   contribution llrintf(value * 2^S) with S = 62 - ceil(log2(H W)) (S - 2 for sum w r^2): no sum can overflow and the result
 *   does not depend on the order of the adds or on the grid.  blocks: workgroups per image, 0 = chosen from the CU count.
 * pf_ego_solve: per image Horn's 4 x 4 matrix of S, its largest eigenvector by cyclic Jacobi in fp64, the quaternion with a
 *   non-negative scalar part, R its matrix; stats [B,5] = {sum w, rms chord sqrt(sum w r^2 / sum w), used / (H W),
 *   gap = (lambda_1 - lambda_2) / sum w, valid}.  valid = 0 when sum w = 0 or gap < gap_min; then R = init (NULL: the identity).
 *   The sums are written back as zeros.  An estimate of k passes is accumulate(weighted = 0, R = init), solve, then k - 1 times
 *   accumulate(weighted = 1, R = the R just solved), solve.
 * pf_ego_track: state [B,8] fp64 = two unit quaternions {O, S} ({1,0,0,0, 1,0,0,0} at the start).  O_t = R_t O_{t-1},
 *   renormalised; S_t = slerp(S_{t-1}, O_t, 1 - smoothing); orient = O_t, corr = O_t S_t^T.  smoothing 1 locks the view to the
 *   first frame (corr = O_t), 0 leaves the video as it is (corr = I).
 * pf_erp_rotate: out(x, y) = in sampled at the ERP position of R s(x, y), four taps, columns wrap, rows clamp; PF_VIEW_F32:
 *   [B,C,H,W] fp32, PF_VIEW_U8: [B,H,W,C] bytes, C = 1..4.
 * pf_ego_derotate: out(x, y) = (ERP position of R^T q) - (x, y), the first component wrapped into [-W/2, W/2); a left-out pixel
 *   gives (0, 0) and valid 0 (valid [B,H,W] bytes or NULL).  out may be flow.
 * PF_ERR_BAD_ARG: a NULL flow / R / sums / stats / state / orient / corr / in / out, sums or state not 8-byte aligned, outputs
 * aliasing each other or an input (but out == flow of pf_ego_derotate), weighted outside {0, 1}, blocks outside 0..65535,
 * scale_px not positive and finite, gap_min negative, smoothing outside [0, 1], C outside 1..4, an unknown form.
 * PF_ERR_BAD_SHAPE: B, H or W < 1, B > 65535, H * W >= 2^30.  Every refusal answers before anything is launched.  One launch
 * each, no host read, no allocation, capturable. */
#define PF_EGO_SUMS 12
#define PF_EGO_STATS 5
#define PF_EGO_STATE 8
long pf_ego_scratch_bytes(int B, int H, int W);
int pf_ego_accumulate(const float* flow, const unsigned char* mask, const float* R, void* sums, int B, int H, int W, int weighted,
                      float scale_px, int blocks, void* stream);
int pf_ego_solve(void* sums, const float* init, float* R, float* stats, int B, int H, int W, float gap_min, void* stream);
int pf_ego_track(const float* R, void* state, float* orient, float* corr, int B, float smoothing, void* stream);
int pf_erp_rotate(const void* in, void* out, const float* R, int B, int C, int H, int W, int form, void* stream);
int pf_ego_derotate(const float* flow, const unsigned char* mask, const float* R, float* out, unsigned char* valid, int B, int H, int W,
                    void* stream);

/* Camera translation from 360-degree flow: the epipole, inverse depth up to the baseline, a mask of what moves (DESIGN.md
 * section 20; the statement is prior-flow_amd/csrc/pf_epipolar.h).  p, q, the left-out rule and the matrices are those of the
 * block above; the model is q ~ R p + kappa t with t a unit vector [B,3] fp32 in DEVICE memory and kappa = |T| / depth >= 0 (a
 * point of the scene moves by T in the second frame's axes; the camera centre moves along -R^T t in the first frame's).
 *
 * pf_epi_accumulate: one pass over flow [B,2,H,W] (mask [B,H,W] bytes or NULL) under R and t (t NULL: the zero vector, mode
 *   PF_EPI_T only) into sums [B,22] int64 (pf_epi_sums_bytes; all-zero before the first pass), integers scaled as
 *   pf_ego_accumulate's.  The weight is cos phi(y) / (1 + e^2 / c^2)^2, e the distance of q from the epipolar great circle of
 *   r = R p under t (0 while t = 0), c = scale_px 2 pi / W.  mode PF_EPI_T adds M = sum w n^ n^T of the votes
 *   n^ = n / sqrt(|n|^2 + c_v^2), n = r x q, c_v = vote_px 2 pi / W, D = sum w d, sum w, sum w e^2, sum w |n|^2 and the count
 *   (sums 0..12); mode PF_EPI_R adds G = sum w g g^T, h = sum w (t . n) g with g = (t . r) q - (r . q) t, sum w and the count (sums
 *   13..21, 9, 12).  blocks: workgroups per image, 0 = chosen from the CU count.
 * pf_epi_solve: mode PF_EPI_T: t = the unit eigenvector of M's smallest eigenvalue (3 x 3 cyclic Jacobi in fp64), turned so that
 *   t . D >= 0; stats [B,6] = {sum w, rms e in pixel widths, used / (H W), gap = (l2 - l1) / (l1 + l2 + l3), parallax rms
 *   sqrt(sum w |n|^2 / sum w) in pixel widths, valid}; valid = 0 when sum w = 0, gap < gap_min or the parallax rms <
 *   min_parallax_px, and then t = t_init (NULL: the zero vector).  R may be NULL.  mode PF_EPI_R: dw = -G^-1 h, R <- exp([dw]x) R in
 *   place; dw = 0 (R untouched) when stats[5] == 0, t = 0 or G's smallest eigenvalue is below 1e-9 of its trace; reads t and
 *   stats.  Either mode writes zeros over the sums it read.
 * pf_epi_map: per pixel conf = |q x t|^2, the signed parallax a = (r x q) . (q x t) / |q x t|, inv_depth = a / |q x t|, resid = |e| in
 *   pixel widths, moving = resid > thr_px or a < -neg_px 2 pi / W; a left-out pixel, conf < conf_min or t = 0 give inv_depth = 0,
 *   resid = 0, moving = 0 (conf as computed, 0 when left out).  Each of the four outputs [B,H,W] may be NULL.
 * PF_ERR_BAD_ARG: a NULL flow / R / sums / t / stats where required, sums not 8-byte aligned, outputs aliasing each other or an
 * input, an unknown mode, blocks outside 0..65535, scale_px or vote_px not positive and finite, a negative or non-finite
 * gap_min / min_parallax_px / thr_px / neg_px / conf_min.  PF_ERR_BAD_SHAPE as above.  Every refusal answers before anything is
 * launched.  One launch each, no host read, no allocation, capturable. */
#define PF_EPI_SUMS 22
#define PF_EPI_STATS 6
#define PF_EPI_T 0
#define PF_EPI_R 1
long pf_epi_sums_bytes(int B, int H, int W);
int pf_epi_accumulate(const float* flow, const unsigned char* mask, const float* R, const float* t, void* sums, int B, int H, int W,
                      int mode, float scale_px, float vote_px, int blocks, void* stream);
int pf_epi_solve(void* sums, const float* t_init, float* R, float* t, float* stats, int B, int H, int W, int mode, float gap_min,
                 float min_parallax_px, void* stream);
int pf_epi_map(const float* flow, const unsigned char* mask, const float* R, const float* t, float* inv_depth, float* resid, float* conf,
               unsigned char* moving, int B, int H, int W, float thr_px, float neg_px, float conf_min, void* stream);

/* Camera trajectory from 360-degree video: the scale link between consecutive pairs, the pose chain and depth fused in one unit
 * (the statement is prior-flow_amd/csrc/pf_odometry.h).  A MAP is what pf_epi_map writes: inv_depth (kappa),
 * conf fp32 [B,H,W] and moving bytes [B,H,W].  Map a and map b lie on ONE grid, the grid of the frame two consecutive pairs share:
 * a of the earlier pair's backward flow under its reversed pose, b of the later pair's forward flow, so kappa_b / kappa_a is the
 * ratio of the two baselines at every static pixel.
 *
 * pf_odo_accumulate: the pixels of both maps into hist [B, 2 bins + 2] int64 (pf_odo_hist_bytes; all-zero before the call).  A pixel
 *   is left out when a moving byte is non-zero, !(conf > 0) or !(kappa_min <= kappa < 2^30) for either map.  Otherwise
 *   w = cos phi(y) min(conf_a, 1) min(conf_b, 1), l = log2(kappa_b / kappa_a) clamped to +-log2_range, bin = floor((l + L) bins /
 *   (2 L)) clamped to 0..bins-1; W[bin] += w, M[bin] += w l / L, total += w (integers scaled by 2^S as pf_ego_accumulate's), count
 *   += 1.  blocks: workgroups per image, 0 = chosen from the CU count.
 * pf_odo_solve: on the integers: the median bin m (the smallest whose inclusive prefix sum C has 2 C >= total), the quartile bins
 *   likewise, l^ = L sum M / sum W over bins m +- trim_bins (cut to the range), ratio [B] = exp2(l^); stats [B,6] = {sum w, used /
 *   (H W), l^, iqr = (q3 - q1) 2 L / bins, window weight / total, valid}.  valid = 0 and ratio = 1 when nothing counted, used / (H W)
 *   < min_used, iqr > max_iqr or m is the first or the last bin.  Every cell is written back as zero.
 * pf_odo_reverse_pose: (R, t) -> (R^T, -R^T t), t = 0 stays +0.
 * pf_odo_track: state [B,12] fp64 = {A (unit quaternion), b[3], S, steps, segment, prev_valid, 0}, {1,0,0,0, 0,0,0, 1, 0,0,0, 0} at
 *   the start.  A <- q(R) A, b <- R b; with pose_stats[5] != 0: S <- S ratio when the pair before was valid and link_stats[5] != 0,
 *   otherwise S stays and segment += 1; then b <- b + S t.  orient [B,3,3] = A, centre [B,3] = -A^T b, baseline [B] = S, flags
 *   [B,4] int32 = {steps, segment, pose valid, link valid}.
 * pf_odo_fuse: a map counts at a pixel where moving == 0, conf >= conf_min and 0 <= kappa < 2^30 (map a only where link_valid[b] !=
 *   0) with weight conf; d = kappa / S; inv_depth = (w_a d_a + w_b d_b) / (w_a + w_b), weight = w_a + w_b, both 0 where nothing counts or the
 *   weight sum is not positive and finite;
 *   disagree = both count, both kappa >= kappa_min and |log2(d_b / d_a)| > tol_log2.  S_a, S_b, link_valid: fp32 [B] in DEVICE
 *   memory.  Each of the three outputs [B,H,W] may be NULL.
 * PF_ERR_BAD_ARG: a NULL input or required output, hist / state not 8-byte aligned, an output whose bytes meet an input's or another
 * output's, bins not a power of two in 64..1024, blocks outside 0..65535, trim_bins outside 0..bins, log2_range / kappa_min / max_iqr /
 * tol_log2 not positive and finite (log2_range at most 64), a negative or non-finite min_used / conf_min.  PF_ERR_BAD_SHAPE as
 * above.  Every refusal answers before anything is launched.  One launch each, no host read, no allocation, capturable. */
#define PF_ODO_STATS 6
#define PF_ODO_STATE 12
#define PF_ODO_FLAGS 4
long pf_odo_hist_bytes(int B, int H, int W, int bins);
int pf_odo_accumulate(const float* inv_a, const float* conf_a, const unsigned char* moving_a, const float* inv_b, const float* conf_b,
                      const unsigned char* moving_b, void* hist, int B, int H, int W, int bins, float log2_range, float kappa_min,
                      int blocks, void* stream);
int pf_odo_solve(void* hist, float* ratio, float* stats, int B, int H, int W, int bins, float log2_range, int trim_bins, float min_used,
                 float max_iqr, void* stream);
int pf_odo_reverse_pose(const float* R, const float* t, float* R_rev, float* t_rev, int B, void* stream);
int pf_odo_track(const float* R, const float* t, const float* pose_stats, const float* ratio, const float* link_stats, void* state,
                 float* orient, float* centre, float* baseline, int* flags, int B, void* stream);
int pf_odo_fuse(const float* inv_a, const float* conf_a, const unsigned char* moving_a, const float* inv_b, const float* conf_b,
                const unsigned char* moving_b, const float* S_a, const float* S_b, const float* link_valid, float* inv_depth,
                float* weight, unsigned char* disagree, int B, int H, int W, float conf_min, float kappa_min, float tol_log2, void* stream);

/* Depth along the trajectory: rigid reprojection of an inverse-depth panorama into the next camera, a z-tested forward splat and a
 * per-pixel recursive depth filter (the statement is prior-flow_amd/csrc/pf_reproject.h).  The convention
 * is the block above's: a scene point X in the earlier frame's axes is R X + T in the later frame's; R [B,9] and T [B,3] fp32 in
 * DEVICE memory, T in the unit of the inverse depth (T = baseline t).
 *
 * pf_reproj_project: per source pixel s = R p + d T, n = |s| (1 when T = 0), d' = d / n, flow = (ERP position of s) - (x, y), the
 *   first component wrapped into [-W/2, W/2).  A pixel is left out (flow 0, d' 0, valid 0) when its mask byte is set (mask [B,H,W]
 *   or NULL), !(weight > 0), !(0 <= d < 2^30) or !(n >= n_min).  flow [B,2,H,W], d_new [B,H,W], valid bytes [B,H,W].
 * pf_zsplat_front / pf_zsplat_accumulate / pf_zsplat_resolve: the STORED flow, d, weight, valid and C = 0..4 payload planes src
 *   [B,C,H,W] (NULL when C = 0) are splatted with pf_splat_accumulate's four taps (columns wrap, rows past a pole are dropped); a
 *   pixel counts when valid != 0, weight > 0, 0 <= d < 2^30 and its landing point and payload values are below 2^30 in magnitude; a
 *   tap is used when its bilinear weight b_k >= b_min.  front [B,H,W] uint32 (all-zero before the call) takes the maximum of the
 *   bit patterns of d over the used taps; accumulate counts a tap iff d 2^tol_log2 >= front there and adds, as 64-bit integers
 *   scaled by pf_splat_accumulate's rule for (1, H, W, max(dmax, vmax)), w_n b_k clamp(src_c, +-vmax), w_n b_k min(d, dmax), w_n b_k
 *   and b_k into acc [B,C+3,H,W] int64 (pf_zsplat_bytes; all-zero before the call), w_n = min(weight, w_max) / w_max.  resolve: hole =
 *   cov < cmin or D <= 0; d_out = N_d / D, w_out = w_max D / cov, out_c = N_c / D (out NULL when C = 0), a hole gives zeros and hole
 *   byte 1; acc and front are written back as zeros.  No result depends on the order of the adds.
 * pf_depth_update: the state (d_s, w_s) [B,H,W] in place from a measurement (d_m, w_m, disagree bytes or NULL), pf_odo_track's flags
 *   [B,4] and the filter's seg [B] int32.  A side counts when its weight is positive and finite and 0 <= d < 2^30 (weights above
 *   w_max are read as w_max); the state not in an image whose flags[1] != seg, the measurement not where disagree is set.  Both, within
 *   |log2(d_m / d_s)| <= tol_log2: the mean weighted by decay w_s and w_m, w = min(decay w_s + w_m, w_max); both, further apart: the
 *   measurement; one: that one (the state's weight decayed); neither: 0, 0.  A second launch then writes seg = flags[1].
 * PF_ERR_BAD_ARG: a NULL input or required output, src / out given with C = 0 or missing with C > 0, C outside 0..4, a pointer not
 * aligned to its element (acc: 8 bytes), an output, acc or front whose bytes meet an input's or another output's, n_min / w_max /
 * cmin / tol_log2 of pf_depth_update not positive and finite, b_min outside [0, 1], tol_log2 of the splat outside [0, 64], decay
 * outside (0, 1], dmax or vmax outside [1, 65536].  PF_ERR_BAD_SHAPE: B, H or W < 1, B > 65535, H * W >= 2^30.  Every refusal
 * answers before anything is launched.  No host read, no allocation, capturable. */
int pf_reproj_project(const float* inv_depth, const float* weight, const unsigned char* mask, const float* R, const float* T, float* flow,
                      float* d_new, unsigned char* valid, int B, int H, int W, float n_min, void* stream);
long pf_zsplat_bytes(int B, int C, int H, int W);
int pf_zsplat_front(const float* src, const float* flow, const float* d, const float* weight, const unsigned char* valid, void* front,
                    int B, int C, int H, int W, float b_min, void* stream);
int pf_zsplat_accumulate(const float* src, const float* flow, const float* d, const float* weight, const unsigned char* valid,
                         const void* front, void* acc, int B, int C, int H, int W, float b_min, float tol_log2, float w_max, float dmax,
                         float vmax, void* stream);
int pf_zsplat_resolve(void* acc, void* front, float* out, float* d_out, float* w_out, unsigned char* hole, int B, int C, int H, int W,
                      float cmin, float w_max, float dmax, float vmax, void* stream);
int pf_depth_update(float* d_s, float* w_s, const float* d_m, const float* w_m, const unsigned char* disagree, const int* flags, int* seg,
                    int B, int H, int W, float tol_log2, float decay, float w_max, void* stream);

/* Moving objects: connected components of a byte mask on the cyclic panorama, per-component sums and a dense, capped object table
 * (the statement is prior-flow_amd/csrc/pf_segments.h).
 *
 * pf_seg_tables: rows [H,2] = (cos phi, sin phi) of every row, cols [W,2] = (cos theta, sin theta) of every column, once per
 *   geometry.  One launch.
 * pf_seg_label: mask bytes [B,H,W] (a pixel is set when its byte is non-zero) into labels int32 [B,H,W]: 1 + the smallest linear
 *   index y W + x of the pixel's component, 0 for background.  connectivity 4 or 8; column W-1 touches column 0 (at 8 also
 *   diagonally); rows do not wrap; with poles = 1 the set pixels of row 0 are one component and so are those of row H-1.  The
 *   labels are a function of the mask alone.  The area sums of the components (cos phi from rows, scaled by 2^32) are left in
 *   scratch for pf_seg_objects.  Three launches.
 * pf_seg_objects: the components of labels (as pf_seg_label left them, with the same scratch) whose area is at least min_area
 *   (equatorial pixels) SURVIVE and are numbered 1, 2, ... by their smallest linear index.  ids int32 [B,H,W]: that number, 0 for
 *   background, for a component that did not survive and for survivors beyond max_objects = M; keep bytes [B,H,W]: 1 on the pixels
 *   of every survivor (those beyond M included); roots int32 [B,M]: the smallest linear index of each object, -1 where unused;
 *   count int32 [B]: the number of survivors, NOT clipped to M; sums int64 [B,M,PF_SEG_SUMS]: area, pixels, cos phi * bearing (3),
 *   value weight, cos phi * value (4) (scales 2^32, 1, 2^32, 2^32, 2^16); table fp32 [B,M,PF_SEG_COLS + C]: area, pixels, centroid
 *   x, y in ERP pixels, resultant length, value weight, C value means; unused rows are zero.  values fp32 [B,C,H,W], C = 0..4 (NULL
 *   when C = 0): a pixel's values count when every channel is below 2^16 in magnitude (a NaN does not).  Five launches.
 * scratch: pf_seg_scratch_bytes(B, H, W) bytes, 8-byte aligned; its contents before a call do not matter.
 * PF_ERR_BAD_ARG: a NULL where one is required, values given with C = 0 or missing with C > 0, C outside 0..4, connectivity not 4
 * or 8, poles not 0 or 1, max_objects outside 1..PF_SEG_MAX_OBJECTS, min_area negative, above 2^30 or NaN, a pointer not aligned
 * to its element (scratch, sums: 8 bytes), scratch_bytes too small, an output or scratch whose bytes meet an input's or another
 * output's.  PF_ERR_BAD_SHAPE: B, H or W < 1, B > 65535, H * W >= 2^30 (beyond which the 64-bit sums could not hold).  Every
 * refusal answers before anything is launched.  No host read, no allocation, capturable. */
#define PF_SEG_SUMS 10
#define PF_SEG_COLS 6
#define PF_SEG_MAX_OBJECTS 4096
long pf_seg_scratch_bytes(int B, int H, int W);
int pf_seg_tables(float* rows, float* cols, int H, int W, void* stream);
int pf_seg_label(const unsigned char* mask, const float* rows, int* labels, void* scratch, long scratch_bytes, int B, int H, int W,
                 int connectivity, int poles, void* stream);
int pf_seg_objects(const int* labels, const float* values, const float* rows, const float* cols, void* scratch, long scratch_bytes,
                   int* ids, unsigned char* keep, int* roots, int* count, float* table, void* sums, int B, int C, int H, int W,
                   int max_objects, float min_area, void* stream);

/* Object tracks: persistent ids for the objects of pf_seg_objects across frames, from flow votes (the
 * statement is prior-flow_amd/csrc/pf_tracker.h).  A push is pf_trk_begin, pf_trk_vote, pf_trk_match, pf_trk_paint: four launches
 * with one flow, five with two.
 *
 * pf_trk_begin: clears votes int64 [B,M,M].
 * pf_trk_vote: every pixel of prev_ids with an id in 1..M follows flow_prev (fp32 [B,2,H,W], on the previous grid, pointing into
 *   the current frame) to the nearest pixel (x cyclic), every pixel of ids follows flow_cur (on the current grid, pointing into
 *   the previous frame); where the target holds an id of the other map the pixel adds its area weight (cos phi of its row from
 *   rows, scaled by 2^32) to votes[prev id - 1][cur id - 1].  Either flow may be NULL, not both.  mask_prev, mask_cur: bytes
 *   [B,H,W] or NULL; a pixel with a non-zero byte, with |u| or |v| not below 2^30 or with a target row outside the image does not
 *   vote.  One launch per flow.
 * pf_trk_match: admissible cells (at least min_overlap * n_dir * the smaller of the two areas, and at least 1), mutual best match
 *   with ties to the smallest index, then per current slot track, age, origin int32 [B,M], step, path fp32 [B,M] and per previous
 *   slot fate int32 [B,M].  count, sums: pf_seg_objects' of the current frame.  The state (st_count [B], st_sums
 *   [B,M,PF_SEG_SUMS], st_track, st_age, st_path [B,M], next_id [B]) is the previous frame's on entry and the current frame's on
 *   return; all of it is read before any of it is written.  A state of zeros with next_id = 1 is the empty one.  n_dir: the number
 *   of flows that voted, 1 or 2.  One launch, one workgroup per image.
 * pf_trk_paint: track_map int32 [B,H,W] = the track of each pixel's object, 0 where ids is 0; st_ids = ids.  One launch.
 * PF_ERR_BAD_ARG: a NULL where a pointer is required or both flows NULL, min_overlap outside (0, 1] or NaN, n_dir not 1 or 2, a
 * pointer not aligned to its element (votes, sums: 8 bytes), an output or a state whose bytes meet an input's or another output's.
 * PF_ERR_BAD_SHAPE: B, H or W < 1, B > 65535, H * W >= 2^30, M outside 1..PF_TRK_MAX_OBJECTS.  Every refusal answers before
 * anything is launched.  No host read, no allocation, capturable. */
#define PF_TRK_MAX_OBJECTS 256
int pf_trk_begin(void* votes, int B, int M, void* stream);
int pf_trk_vote(const int* prev_ids, const int* ids, const float* flow_prev, const float* flow_cur, const unsigned char* mask_prev,
                const unsigned char* mask_cur, const float* rows, void* votes, int B, int H, int W, int M, void* stream);
int pf_trk_match(const void* votes, const int* count, const void* sums, int* st_count, void* st_sums, int* st_track, int* st_age,
                 float* st_path, int* next_id, int* track, int* age, int* origin, int* fate, float* step, float* path, int B, int M,
                 int n_dir, float min_overlap, void* stream);
int pf_trk_paint(const int* ids, const int* track, int* track_map, int* st_ids, int B, int H, int W, int M, void* stream);

/* Push-pull hole filling on the cyclic panorama (the statement is prior-flow_amd/csrc/pf_fill.h): a weighted
 * pyramid of what is known (pull, 2 x 2 blocks, no wrap), expanded back (push, bilinear, columns wrapped, rows clamped) and taken
 * only where the finer level knows nothing.  Gather only: the same bits on every run.
 *
 * src fp32 [B,C,H,W], C = 1..4; hole uint8 [B,H,W], non-zero: missing; weight fp32 [B,H,W] or NULL: a soft weight, cut to [0, 1].
 * A pixel whose values are not finite (or at or beyond 2^30 in magnitude) or whose weight is not finite or <= 0 counts as a hole.
 * pf_fill_levels: the number of pulls L until the level is 1 x 1 (H_(l+1) = max(1, ceil(H_l / 2))), or PF_ERR_BAD_SHAPE.
 * pf_fill_bytes: the bytes of scratch for the shape (w0 [B,H,W], then per level l = 1..L the values [B,C,H_l,W_l] and the weights
 *   [B,H_l,W_l], all fp32), or a negative PF_ERR_* code.  scratch needs no initialisation and is private to a call until it ends.
 * pf_fill_pushpull: out fp32 [B,C,H,W] = src with its holes closed (a valid pixel of weight 1 keeps its bits), empty uint8 [B] or
 *   NULL = 1 where an image has nothing valid (its out is 0).  Three launches when the levels above the fifth fit the apex kernel's
 *   LDS (about 600 000 pixels at C = 4), two more per level beyond.  out may be exactly src.
 * The level-by-level form, one launch each, the same bits: pf_fill_prepare writes w0 [B,H,W]; pf_fill_pull_level the level above
 *   (coarse_v [B,C,Hc,Wc], coarse_w [B,Hc,Wc], Hc = max(1, ceil(Hf / 2))) of (fine_v [B,C,Hf,Wf], fine_w [B,Hf,Wf]);
 *   pf_fill_push_level out [B,C,Hf,Wf] from the filled level above coarse_u [B,C,Hc,Wc]; out may be exactly fine_v.  At the 1 x 1
 *   level coarse_u is NULL: the apex step, which alone may write empty.
 * PF_ERR_BAD_ARG: a NULL where a pointer is required, a float map not aligned to 4 bytes, C outside 1..4, an output or scratch whose
 * bytes meet an input's or another output's (other than out == src / out == fine_v), coarse_u given at the 1 x 1 level or missing
 * elsewhere, empty given elsewhere.  PF_ERR_BAD_SHAPE: B, H or W < 1, B > 65535, H * W >= 2^30, a pull of the 1 x 1 level.  Every
 * refusal answers before anything is launched.  No atomics, no memset, no host read, no allocation, capturable. */
int pf_fill_levels(int H, int W);
long pf_fill_bytes(int B, int C, int H, int W);
int pf_fill_pushpull(const float* src, const unsigned char* hole, const float* weight, float* out, unsigned char* empty, void* scratch,
                     int B, int C, int H, int W, void* stream);
/* One stage of pf_fill_pushpull alone, on a scratch that a whole call has filled: 0 the pull tiles, 1 the apex kernel (with the
 * level-by-level launches around it on a large map), 2 the push tiles.  For timing (profiles/time_fill.py) and for a test of the
 * split: the three stages in order are pf_fill_pushpull.  PF_ERR_BAD_ARG: another stage. */
int pf_fill_stage(const float* src, const unsigned char* hole, const float* weight, float* out, unsigned char* empty, void* scratch,
                  int B, int C, int H, int W, int stage, void* stream);
int pf_fill_prepare(const float* src, const unsigned char* hole, const float* weight, float* w0, int B, int C, int H, int W, void* stream);
int pf_fill_pull_level(const float* fine_v, const float* fine_w, float* coarse_v, float* coarse_w, int B, int C, int Hf, int Wf,
                       void* stream);
int pf_fill_push_level(const float* coarse_u, const float* fine_v, const float* fine_w, float* out, unsigned char* empty, int B, int C,
                       int Hf, int Wf, void* stream);

/* flow = coords1 - coords_grid (core/prior_raft.py:172,177).  coords1: planar.  flow_out
 * (planar) and the two channel-last destinations are optional (NULL to skip). */
int pf_flow_prep(const float* coords1, float* flow_out,
                 float* d0, int d0_ld, int d0_off, float* d1, int d1_ld, int d1_off,
                 int B, int H8, int W8, void* stream);

/* flo_rotate (core/utils/projection_prim_ortho.py:531-546 + core/utils/my_cycle_sample.py:6-97):
 * express a flow field of one view in the other view.  flow/out: planar. */
int pf_flo_rotate(const float* flow, const float* g_w2c, const float* g_c2w, float* out,
                  float* d0, int d0_ld, int d0_off, float* d1, int d1_ld, int d1_off,
                  int B, int H8, int W8, void* stream);

/* ---- correlation volume, pyramid, lookups ---------------------------------------------- */

/* PriOr_RAFT.corr + DCCL.build_pyramid (core/prior_raft.py:69-75, core/corr.py:99-111), fused:
 * level0[b][n1][n2] = <f1[b][n1][:], f2[b][n2][:]> / sqrt(C); level i+1 = 2x2 mean of level i
 * over (y2,x2).  f1,f2: channel-last [B*N][C] (C % 32 == 0).  lvl[i]: [B*N][(H8>>i)*(W8>>i)].
 * Any H8, W8 >= 16 (odd levels pool with floor semantics, like avg_pool2d).  Maps with W8 % 32 == 0 and H8 % 8 == 0
 * take the fused kernel that writes all four levels in one pass (at B >= 4 and W8 % 64 == 0 its LDS-DMA ring
 * form); other maps take a generic corr kernel + three pooling passes.  PF_ERR_BAD_SHAPE: C % 32 != 0 or a map
 * whose row offsets do not fit 32 bits. */
int pf_corr_pyramid(const float* f1, const float* f2, float* lvl0, float* lvl1, float* lvl2,
                    float* lvl3, int B, int H8, int W8, int C, void* stream);

/* Same as pf_corr_pyramid in the 3-pass bf16 split arithmetic (hi*hi + hi*lo + lo*hi, fp32 accumulate):
 * f1_split / f2_split are the feature rows pre-split by pf_split_bf16. */
int pf_corr_pyramid_bf16x3(const void* f1_split, const void* f2_split, float* lvl0, float* lvl1,
                           float* lvl2, float* lvl3, int B, int H8, int W8, int C, void* stream);

/* fp32 rows [rows][C] -> bf16 hi|lo split rows [rows][C/32]{hi[32], lo[32]} (C % 32 == 0): the operand
 * format of the PF_PREC_BF16X3 GEMMs.  hi = bf16(x) round-to-nearest-even, lo = bf16(x - hi). */
int pf_split_bf16(const float* in, void* out, long rows, int C, void* stream);

/* fp32 rows [rows][ld_in] (channels 0..C) -> f16 map [rows][lds_out x 128 B] (see PF_PREC_F16), fp16 round to nearest even;
 * columns >= C are not written.  C % 4 == 0.  The context features net / inp of cnet (core/prior_raft.py:134-142) once per
 * forward when the update blocks run in fp16 (mixed_precision: the autocast region core/prior_raft.py:190). */
int pf_split_f16(const float* in, int ld_in, void* out, int lds_out, long rows, int C, void* stream);

/* Training: the packed weight / bias gradients of several convolutions (pf_conv2d_wgrad's dw / db) added into the parameters'
 * own gradient tensors, PF_UNPACK_MAX_JOBS (16) convolutions per launch -- what optimizer-side autograd does per parameter with
 * a permute copy, a clone and two accumulation adds (train_flow.py:135 loss.backward() on the reference):
 *   gw[o][c][tap] += scale * dw[o_off + o][tap][c]   (gw: [cout][cin][kh][kw], taps = kh*kw)      gb[o] += scale * db[o_off + o]
 * o_off: first packed row of this module inside a fused convolution (convz|convr); gb / db may be NULL together. */
typedef struct pf_unpack_job {
    const float* dw; const float* db; float* gw; float* gb;
    int cout, cin, taps, cin_pad, o_off; float scale;
} pf_unpack_job;
int pf_unpack_wgrads(const pf_unpack_job* jobs, int n, void* stream);

/* nn.Conv2d weights -> the PF_PREC_BF16X3 operand format of pf_conv2d, on the device, in one launch (what a training step
 * does for every convolution after each optimizer step, train_flow.py:138-140; replaces ~9 PyTorch-ROCm kernels per pack).
 * w0 [cout0][cin][kh][kw] and optionally w1 [cout1][cin][kh][kw] concatenated on the output channels (the fused z|r
 * convolution of core/update.py:48-49); b0 / b1 their biases (NULL = zero).
 *   mode 0: forward convolution: dst_w [cout_pad][kh*kw][cin_pad/32] x {bf16 hi[32], bf16 lo[32]}, dst_b [cout_pad].
 *   mode 1: its data-gradient convolution (pf_conv2d_wgrad's comment): W'[c][o][ky][kx] = W[o][(c + cin_rot) % cin][kh-1-ky][kw-1-kx],
 *           i.e. packed output channels = forward input channels rotated by cin_rot, packed input channels = forward output
 *           channels; dst_b (optional) is zeroed.
 * Padding rows / columns are written as zeros: dst needs no initialisation. */
int pf_pack_conv_weights(const float* w0, int cout0, const float* w1, int cout1, const float* b0, const float* b1,
                         int cin, int kh, int kw, int mode, int cin_rot, void* dst_w, float* dst_b,
                         int cout_pad, int cin_pad, void* stream);
/* Several of them per launch (16 jobs each; the arguments of pf_pack_conv_weights as a struct).  The jobs of one launch are
 * validated just before that launch: when a bad job is reported (PF_ERR_BAD_ARG / PF_ERR_BAD_SHAPE), the launches before its own
 * -- the first 16 jobs for a bad job at index 17 -- have already been enqueued, and no job of its own launch or after it has. */
typedef struct pf_pack_job {
    const float* w0; const float* w1; const float* b0; const float* b1; void* dst_w; float* dst_b;
    int cout0, cout1, cin, kh, kw, mode, cin_rot, cout_pad, cin_pad;
} pf_pack_job;
int pf_pack_conv_weights_batch(const pf_pack_job* jobs, int n, void* stream);

/* DCCL.__call__ steps 1-2 (core/corr.py:119-137): own-view 9x9x4 lookup and the raw
 * cross-view lookup through g_w2c.  coords: planar.  own_out/raw_out: channel-last, 324
 * channels = level*81 + a*9 + b (x += a-4, y += b-4), row stride ld >= 324. */
int pf_dccl_lookup(const float* coords,
                   const float* own0, const float* own1, const float* own2, const float* own3,
                   const float* oth0, const float* oth1, const float* oth2, const float* oth3,
                   const float* g_w2c, float* own_out, float* raw_out,
                   int B, int H8, int W8, int ld, void* stream);

/* pf_dccl_lookup with an additional copy of the grid interleaved per pixel, g_w2c_il [H8*W8][2] = (x, y): the two
 * components of a bilinear row pair become one 16-byte load (the kernel is bound by its gather-instruction count).
 * g_w2c_il may be NULL (= pf_dccl_lookup).  Results are bit-identical either way. */
int pf_dccl_lookup_il(const float* coords,
                      const float* own0, const float* own1, const float* own2, const float* own3,
                      const float* oth0, const float* oth1, const float* oth2, const float* oth3,
                      const float* g_w2c, const float* g_w2c_il, float* own_out, float* raw_out,
                      int B, int H8, int W8, int ld, void* stream);

/* alternate_corr (AlternateCorrBlock, core/corr.py:64-91): the lookups without the correlation volumes.
 *
 * pf_feature_pyramid: levels 1-3 of f2 pooled, channel-last [B*N_i][C] rows, N_i = (H8>>i)*(W8>>i).  Level i+1 is
 * the 2x2 mean of level i with avg_pool2d floor semantics (odd sizes drop the last row / column).  Level 0 is f2.
 *
 * pf_dccl_lookup_feat: the outputs of pf_dccl_lookup(coords, pyr(f1_own, f2_own), pyr(f1_oth, f2_oth), g_w2c, ...),
 * up to rounding, computed from the features: level i of the pyramid at (n, p) is <f1[n], P_i(f2)[p]> / sqrt(C), so
 * every bilinear corner is one C-long fp32 dot product at lookup time.  f1_* / f2_*0: channel-last [B*N][C];
 * f2_*1..3: pf_feature_pyramid's levels.  Same 324-channel layout, row stride ld >= 324 (columns >= 324 are not
 * written) and semantics: x wrapped mod W_i then zero padded; the cross view samples the LEVEL-0 grid at level-i
 * coordinates and uses the result un-scaled at level i; raw row n correlates the OTHER branch's f1[n].
 * path_counts: NULL, or a device int[2] the kernel adds to: (tile, level, view) units whose corners were computed from
 * window rows staged in LDS once per tile of neighbouring pixels [0], or per pixel from global memory [1] (the host
 * emulation leaves it untouched).
 * Both: C % 4 == 0, C <= 512, level 3 at least 2x2, feature pointers 16-byte aligned. */
int pf_feature_pyramid(const float* f2, float* l1, float* l2, float* l3, int B, int H8, int W8, int C, void* stream);
int pf_dccl_lookup_feat(const float* coords, const float* f1_own,
                        const float* f2_own0, const float* f2_own1, const float* f2_own2, const float* f2_own3,
                        const float* f1_oth,
                        const float* f2_oth0, const float* f2_oth1, const float* f2_oth2, const float* f2_oth3,
                        const float* g_w2c, float* own_out, float* raw_out, int* path_counts,
                        int B, int H8, int W8, int C, int ld, void* stream);


/* DCCL.__call__ step 3 + the caller's add (core/corr.py:138, core/prior_raft.py:187-188):
 * out = own + img_rotate(raw, g_back), channel-last. */
int pf_dccl_combine(const float* own, const float* raw, const float* g_back, float* out,
                    int B, int H8, int W8, int ld, int ld_out, void* stream);

/* cycle_bilinear_sampler + groupwise_corr (core/prior_raft.py:173-174,180-182,77-83):
 * dst[.., c_off+g] = mean_{c in group g} f1[c] * warp(f2, coords)[c], 4 groups.
 * coords planar; if add_grid != 0 it is a flow and coords0 is added first. */
int pf_warp_gcorr(const float* f1, const float* f2, const float* coords, int add_grid,
                  float* dst, int dst_ld, int dst_off, int B, int H8, int W8, int C, void* stream);

/* Motion inputs of one refinement iteration in one launch (core/prior_raft.py:171-182): flow_A = coords1_A - coords0,
 * flow_B = coords1_B - coords0, flow_B_A = flo_rotate(flow_B, W2C = grid(R_A2B), C2W = grid(R_B2A)), and the two
 * groupwise correlations flaw_A = gwc(f1A, warp(f2A, coords1_A)), flaw_B_A = gwc(f1A, warp(f2A, coords0 + flow_B_A)).
 * Bit-identical to pf_flow_prep x2 + pf_flo_rotate + pf_warp_gcorr x2.  Outputs: flow4_a [B*N][4] = flow_A | flow_B_A,
 * flow2_b [B*N][2]; optional GRU-input tails xa (4 columns at xa_off) / xb (2 columns at xb_off); conf [B*N][conf_ld]
 * columns 0..3 flaw_A, 4..7 flaw_B_A.  C must be 256.  xa_split / xb_split (with xa_lds / xb_lds chunks per row): optional
 * split twins (see pf_conv_desc) of the GRU-input buffers, tails written at the same channel offsets xa_off / xb_off. */
int pf_motion_prep(const float* c1a, const float* c1b, const float* g_w2c, const float* g_c2w,
                   const float* f1a, const float* f2a, float* flow4_a, float* flow2_b,
                   float* xa, int xa_ld, int xa_off, float* xb, int xb_ld, int xb_off,
                   void* xa_split, int xa_lds, void* xb_split, int xb_lds,
                   float* conf, int conf_ld, int B, int H8, int W8, int C, void* stream);
/* The same with the GRU-input tails written to f16 maps (PF_PREC_F16; xa_lds / xb_lds units of 64 channels per row) instead of
 * split twins: the fp16 update blocks of mixed_precision (core/prior_raft.py:190, core/update.py:155,133). */
int pf_motion_prep_f16(const float* c1a, const float* c1b, const float* g_w2c, const float* g_c2w,
                       const float* f1a, const float* f2a, float* flow4_a, float* flow2_b,
                       float* xa, int xa_ld, int xa_off, float* xb, int xb_ld, int xb_off,
                       void* xa_f16, int xa_lds, void* xb_f16, int xb_lds,
                       float* conf, int conf_ld, int B, int H8, int W8, int C, void* stream);

/* Confidence stem of the ODDC motion encoder in one launch (core/update.py:177-178,193-194):
 * out[.., off_out .. off_out+16) = relu(conv3x3_{32->16}(relu(conv3x3_{8->32}(in[.., off_in .. off_in+8))))), zero padding,
 * exact fp32; w1 [9*8][32], w2 [9*32][16] in the [KH*KW][Cin][Cout] packing of pf_conv2d_direct.  The 32-channel
 * intermediate map never leaves LDS.  out_split / lds_out: optional split twin of `out` (see pf_conv_desc) written at the
 * same channel offset (% 4 == 0); `out` may then be NULL. */
int pf_conf_stem(const float* in, int ld_in, int off_in, const float* w1, const float* b1,
                 const float* w2, const float* b2, float* out, int ld_out, int off_out,
                 void* out_split, int lds_out, int B, int H8, int W8, void* stream);
/* The same, writing an f16 map (PF_PREC_F16) instead of the split twin: the input of conv_A in the autocast region of
 * mixed_precision (core/prior_raft.py:190, core/update.py:193-201).  Exact fp32 arithmetic as before. */
int pf_conf_stem_f16(const float* in, int ld_in, int off_in, const float* w1, const float* b1,
                     const float* w2, const float* b2, float* out, int ld_out, int off_out,
                     void* out_f16, int lds_out, int B, int H8, int W8, void* stream);

/* ---- update blocks ------------------------------------------------------------------------ */

/* Epilogues of pf_conv2d. */
#define PF_EPI_LINEAR 0   /* out = (acc + bias) * scale                                   */
#define PF_EPI_RELU 1     /* out = relu(acc + bias)                                       */
#define PF_EPI_GRU_ZR 2   /* cout [0,128): out = sigmoid(.) -> z; [128,256): aux_out = sigmoid(.)*h */
#define PF_EPI_GRU_Q 3    /* q = tanh(.); out = (1-z)*h + z*q                              */
#define PF_EPI_TANH_RELU 4 /* cout [0,128): out = tanh(.); [128,256): aux_out = relu(.)
                            * (net / inp split of the context features, core/prior_raft.py:136-142) */
#define PF_EPI_RELU_RES 5  /* out = relu(res + relu(acc + bias)), res = h[.., j] (ld_h): the tail of a ResidualBlock whose
                            * norm2 is an eval-mode BatchNorm folded into the weights (core/extractor.py:41-47) */
#define PF_EPI_MASK 6      /* out = h[.., j] > 0 ? (acc + bias) * scale : 0 -- the data gradient of a convolution whose INPUT was
                            * a ReLU output y (h = y, ld_h): dgrad and the ReLU's backward in one launch (training, train_flow.py:135) */
#define PF_EPI_ADD 7       /* out = (acc + bias) * scale + h[.., j] (ld_h; out may alias h): a data gradient accumulated into the
                            * gradient another consumer of the same tensor has already left there */

/* Arithmetic of pf_conv2d (pf_conv_desc.precision); the weight buffer format follows it. */
#define PF_PREC_F32 0     /* exact fp32 MFMA; weights fp32 [Cout_pad][KH*KW][Cin_pad]                 */
#define PF_PREC_BF16X3 1  /* 3-pass bf16 split (hi*hi + hi*lo + lo*hi), fp32 accumulate; weights     *
                           * pre-split: [Cout_pad][KH*KW][Cin_pad/32] x {bf16 hi[32], bf16 lo[32]}  */
#define PF_PREC_F16 2     /* single-pass fp16 operands, fp32 accumulate, bias / epilogue / outputs fp32: the update blocks
                           * under CUDA autocast (mixed_precision, core/prior_raft.py:190; core/update.py).  Weights fp16
                           * [Cout_pad][KH*KW][Cin_pad64] (Cin_pad64 = c0 + c1 rounded up to 64).  Operands are F16 MAPS only:
                           * in0_split / in1_split / out_split / aux_split then denote channel-last fp16 rows of lds x 128 bytes
                           * (64 channels per unit, channel c at byte 2c of the row, zero past the logical width -- a padded
                           * float16 tensor [rows][lds * 64]); fp16 = round to nearest even of the producer's fp32 value.
                           * off0 / off1 (and c0 with in1) must be multiples of 64, a last segment ending inside a 64-channel
                           * unit must end at its row's end, every group of a launch is F16, and the launch must be one the
                           * all-DMA kernel takes (stride-1 3x3 / 1x5 / 5x1, no in_scale / stats_out): PF_ERR_BAD_SHAPE /
                           * PF_ERR_BAD_ARG otherwise, never a fallback.  pf_conv2d_tile / _roles / _stats_blocks report
                           * the plan of an F16 launch like any other. */

/* One stride-1 "same" convolution on channel-last activations as an implicit GEMM on the
 * matrix cores (nn.Conv2d forwards of core/update.py:6-14, 35-60, 81-99, 117-136, 139-201).
 * The input is the virtual concatenation of two channel-last segments (in1 may be NULL);
 * c0 must be a multiple of 32 when in1 is used.  Weights are pre-packed
 * [Cout_pad][KH*KW][Cin_pad] (Cin_pad = c0 + c1 rounded up to 32, Cout_pad to 128, zero filled).
 */
typedef struct pf_conv_desc {
    const float* in0; int ld0; int off0; int c0;
    const float* in1; int ld1; int off1; int c1;
    const float* weight; const float* bias;
    float* out; int ld_out; int off_out; int cout;
    int kh, kw;
    int epilogue; float scale;
    const float* h; int ld_h;        /* GRU_ZR / GRU_Q: hidden state [B*N][ld_h]            */
    const float* z; int ld_z;        /* GRU_Q: update gate                                  */
    float* aux_out; int ld_aux;      /* GRU_ZR: r*h                                         */
    int precision;                   /* PF_PREC_*; identical in every group of a launch     */
    int stride;                      /* 1 or 2; input map = stride x the output map         */
    /* optional per-(image, input-channel) affine + ReLU applied to the INPUT as it is loaded
     * (the previous layer's Instance/BatchNorm folded into this conv): x' = relu?(x*s + t).
     * [B][c0+c1] floats each; NULL = none.  Halo-kernel convolutions only (3x3/1x5/5x1, bf16x3). */
    const float* in_scale; const float* in_shift; int in_relu;
    /* optional InstanceNorm statistics of THIS conv's output, fused into its epilogue (PF_EPI_LINEAR only):
     * stats_out[((image*nblk + tile)*cout + c)*2 + {0,1}] = fp64 sum / sum of squares of output channel c over one workgroup
     * tile.  nblk = pf_conv2d_stats_blocks(...).  Halo-kernel tiles 3/4/5/8: nblk = tiles per image = ceil(H8/TH)*ceil(W8/32), TH = 8 for
     * tiles 5 and 8 else 4; tile 6: one partial per (segment of rows, row phase of the 4-row step, strip).  Generic
     * kernel (pf_conv2d_tile 0/1/2/7, bf16x3; the stride-2 layers): tiles of BM = 128/64/64/128 consecutive pixels, nblk = H8*W8/BM,
     * which must divide (PF_ERR_BAD_SHAPE otherwise).  Finish with pf_channel_stats_final.  NULL = none. */
    double* stats_out;
    /* Pre-split activations (PF_PREC_BF16X3 only).  A "split twin" of a channel-last map holds, per pixel row and per
     * 32-channel chunk, the 128 bytes {bf16 hi[32], bf16 lo[32]} with hi = bf16(x) (round to nearest even) and
     * lo = bf16(x - hi): [rows][lds chunks][128 B] -- exactly what the kernels otherwise compute from fp32 while staging,
     * so results are bit-identical.  Channels past the logical width of a row are zero.
     *   in0_split / in1_split (with lds0 / lds1 chunks per row; off0 / off1 / c0 must be multiples of 32; a last segment whose
     *     width is not a multiple of 32 must end at the end of its twin's row -- the kernel copies whole chunks and relies on
     *     the zero columns past the logical width, PF_ERR_BAD_SHAPE otherwise): when EVERY group of
     *     a stride-1 3x3 / 1x5 / 5x1 launch without in_scale / stats_out provides them, the operands go global -> LDS by DMA
     *     (pf_conv_dma_kernel: no VALU split, no ds_write) and in0 / in1 may be NULL; other launches ignore them and need in0.
     *   out_split (lds_out chunks per row; off_out % 32 == 0): the epilogue also writes the split twin of `out` at the same
     *     channel offset; `out` may then be NULL (twin only).  aux_split / lds_aux: the same for `aux_out` (GRU_ZR: r*h,
     *     TANH_RELU: inp).  Any kernel form honours the output twins. */
    const void* in0_split; int lds0;
    const void* in1_split; int lds1;
    void* out_split; int lds_out;
    void* aux_split; int lds_aux;
    /* with in0_split: a block of at least 128 * max(lds0, lds1) zero bytes (16-byte aligned) -- what the all-DMA kernel
     * reads for the zero padding around the map (an LDS-DMA copies memory; it cannot write a constant) */
    const void* zeros; int zeros_bytes;
    /* Optional start value of the accumulation (all-DMA kernel only; any other kernel form answers PF_ERR_BAD_SHAPE):
     * channel-last fp32 [B*N][ld_pre], output channel j of this conv at column off_pre + j.  The accumulators start from
     * pre instead of zero, so out = epilogue(pre + conv(in) + bias).  Used for the iteration-invariant part of the GRU
     * convolutions: the context features `inp` are the same in all `iters` iterations (core/prior_raft.py:148,196), so
     * conv_{[h|inp|motion]} = conv_inp(inp) [computed once] + conv_{[h|motion]} [per iteration, 2/3 of the MFMA work]. */
    const float* pre; int ld_pre; int off_pre;
    /* Training forward (the gate values are operands of pf_gru_zr_bwd / pf_gru_q_bwd): with save_gates != 0 and aux_out set,
     * PF_EPI_GRU_ZR also writes r = sigmoid(.) to aux_out[.., 128 + j'] (j' = j - 128; r*h stays at aux_out[.., j'], so
     * ld_aux >= 256) and PF_EPI_GRU_Q also writes q = tanh(.) to aux_out[.., j] (ld_aux >= 128). */
    int save_gates;
    /* Tile-choice hint (descs[0] of a launch): the number of further launches of the same geometry the caller runs BESIDE this one
     * on other streams (round 6: branch A's and branch B's update blocks as two chains, core/prior_raft.py:196-211).  The host
     * counts work items as if those launches' groups were groups of this one, so two half-chip launches keep the tile a
     * two-group launch takes instead of falling back to the smaller tile that would fill the chip alone.  0 = none. */
    int co_groups;
} pf_conv_desc;

/* The tail of DCCL.__call__ fused with the first motion-encoder convolution (core/corr.py:138,
 * core/prior_raft.py:187-188, core/update.py:185 / :92), PF_PREC_BF16X3 arithmetic:
 *   out[.., off_out .. off_out+256) = relu(conv1x1_{324->256}(own + img_rotate(raw, g_back)))
 * own, raw: channel-last [B*N][ld] outputs of pf_dccl_lookup; weight: the pf_conv2d packing of the 1x1 conv
 * (pre-split bf16 [256][1][11] x {hi[32], lo[32]}); cout must be 256.  Bit-identical to pf_dccl_combine followed by
 * pf_conv2d, but the combined 324-channel tensor is never written. */
typedef struct pf_combine_conv_desc {
    const float* own; const float* raw; int ld;
    const float* g_back;               /* [2][N] rotate-back grid */
    const void* weight; const float* bias;
    float* out; int ld_out; int off_out; int cout;
    void* out_split; int lds_out;      /* optional split twin of `out` (see pf_conv_desc), same channel offset (% 32 == 0);
                                        * `out` may then be NULL */
} pf_combine_conv_desc;
/* ngroups = 1 | 2: branch A and branch B of an iteration in one launch (grid.y = group). */
int pf_dccl_combine_conv1x1(const pf_combine_conv_desc* descs, int ngroups, int B, int H8, int W8, void* stream);
/* The same launch (bf16x3 arithmetic) with out_split an f16 map (PF_PREC_F16, lds_out units of 64 channels): convc1's output
 * as the operand of the fp16 convc2 under mixed_precision (core/prior_raft.py:190, core/update.py:185-186 / :92-93). */
int pf_dccl_combine_conv1x1_f16(const pf_combine_conv_desc* descs, int ngroups, int B, int H8, int W8, void* stream);

/* Launch `ngroups` (1..4) same-geometry convolutions in ONE kernel (grid.z = group):
 * branch A and branch B of an iteration run side by side.  H8, W8 = OUTPUT map size. */
int pf_conv2d(const pf_conv_desc* descs, int ngroups, int B, int H8, int W8, void* stream);

/* Host-only queries: pf_conv2d plans every launch once (validation, tile, kernel instantiation, wave organisation, statistics
 * blocks) and runs that plan; each query computes the same plan and returns one field of it, or the negative PF_ERR_* code with
 * which pf_conv2d refuses the descriptors.  They launch nothing and need no GPU.
 *
 * pf_conv2d_tile: the workgroup tile of the launch -- generic kernel 0: 128x32, 1: 64x64, 2: 64x128, 7: 128x96 (pixels x
 * channels; 7 = round 6, for the 96 output channels of the encoders' layer 2); halo kernel 3: 128x64, 4: 128x128, 5: 256x64
 * (8-row tile), 8: 256x96 (8-row tile, 3x3 with 64 < Cout <= 96; round 6); 6: the weights-stationary kernel of the encoders'
 * 3x3 64 -> 64 convolutions (round 5; core/extractor.py:16-17 at 1/2 resolution: strips of 32 columns walked in 4-row steps,
 * outputs bit-identical to tile 5).  A 3x3 launch of the all-DMA kernel (pf_conv2d_roles >= 16) on tiles 3 / 4 reports the
 * channel half of its tile here -- 3: NT = 1, 4: NT = 2 (32 * NT channels per MFMA wave) -- and the pixel half in the roles
 * code.  Lets a profiler attribute measured time to the right kernel instantiation. */
int pf_conv2d_tile(const pf_conv_desc* descs, int ngroups, int B, int H8, int W8);

/* pf_conv2d_stats_blocks: how many fp64 partial blocks PER IMAGE the launch writes to `stats_out` (the nblk of
 * pf_channel_stats_final and of the buffer's size, [B][nblk][cout][2] doubles), answered for the launch with `stats_out` set;
 * 0 = the launch cannot fuse the statistics (generic kernel whose pixel tiles would straddle images, or not bf16x3). */
int pf_conv2d_stats_blocks(const pf_conv_desc* descs, int ngroups, int B, int H8, int W8);

/* pf_conv2d_roles: the wave organisation of the launch.  Nonzero only with tiles 3, 4, 5 and 8; 0 on every other tile
 * (the generic kernel, the weights-stationary kernel 6) --
 * 0: every wave stages and multiplies (pf_conv_halo_kernel), 1: four MFMA waves + four loader waves on the same tile
 * (pf_conv_ws_kernel<NT, KH, KW, 2>; tiles 3 / 4), 2: the same with a 256 px x 64 channel tile (pf_conv_ws_kernel<2, KH, KW, 1>;
 * tiles 3 / 4); 16 + 1 | 16 + 2: the launch has pre-split operands and takes the all-DMA kernel (pf_conv_dma_kernel) with
 * the 128-pixel | a 256-pixel tile (tiles 3, 4, 5, 8; tile 5 always with 16 + 2).  3x3 on tiles 3 / 4: the tile is the one whose
 * busiest workgroup stages the fewest bytes, and the two codes name the instantiation --
 * tile 3, 16 + 1: pf_conv_dma_kernel<1,3,3,2> 128 px x 64 channels;   tile 3, 16 + 2: <1,3,3,1> 256 px x 32 channels;
 * tile 4, 16 + 1: <2,3,3,2> 128 px x 128 channels;                    tile 4, 16 + 2: <2,3,3,1> 256 px x 64 channels.
 * (1x5 / 5x1, and every launch under PRIORFLOW_DMA_TALL=0 -- an A/B knob read once per process that restores the tile choice
 * before that rule --, report 16 + 2 for <2,KH,KW,1> on whichever of the tiles 3 / 4 the work-item count gave.) */
int pf_conv2d_roles(const pf_conv_desc* descs, int ngroups, int B, int H8, int W8);

/* The encoders' first convolution (core/extractor.py:122, :144: conv1 7x7 stride 2 pad 3, 3 -> 64) straight from the NCHW
 * image, PF_PREC_BF16X3 arithmetic on the matrix cores with K = the 7x7x3 patch (176 padded) instead of the 512 of the
 * space-to-depth form: img [Bn][3][H][W] (H, W even) -> out rows [Bn * H/2 * W/2][64] fp32 (may be NULL with out_split) and / or
 * the split twin out_split [rows][2 chunks][128 B] (see pf_conv_desc); relu != 0: ReLU epilogue (the BatchNorm-folded cnet
 * stem).  weight: 64 rows of 704 bytes -- per 8-k piece {bf16 hi[8], bf16 lo[8]}, k = ky * 24 + kx * 3 + c, zero padded
 * (engine.pack_stem7x7 builds it); bias [64].  stats_out (optional): fp64 per-tile sum / sum of squares of the stored values,
 * [Bn][ceil(H/16) * ceil(W/64)][64][2] -- the partials pf_channel_stats_final reduces (8-row x 32-column output tiles). */
int pf_enc_stem(const float* img, const void* weight, const float* bias, float* out, void* out_split, int relu,
                double* stats_out, int Bn, int H, int W, void* stream);

/* Test support (tests/test_hip_kernels.py): fills the whole 160 KB LDS of every CU with `pattern` (e.g. 0x7fc00000, a NaN), so
 * that a kernel which reads LDS it never wrote -- padding floats multiplied by zero weights -- shows up as NaNs in its output.
 * No counterpart in the reference. */
int pf_debug_dirty_lds(unsigned pattern, void* stream);

/* Tiny-Cin direct convolution (7x7 2->128, 3x3 8->32, 3x3 32->16; core/update.py:171-178,87).
 * Weights packed [KH*KW][Cin][Cout]. */
int pf_conv2d_direct(const float* in, int ld_in, int off_in, int cin,
                     const float* weight, const float* bias,
                     float* out, int ld_out, int off_out, int cout,
                     int kh, int kw, int relu, int B, int H8, int W8, void* stream);

/* The same convolution for 1..4 independent problems of one shape in ONE launch (the motion encoders' 7x7
 * stems of flow_A, flow_B_A and flow_B, core/update.py:187-188,:94, read three different 2-channel inputs).
 * Outputs must not overlap. */
typedef struct pf_direct_desc {
    const float* in;  int ld_in, off_in;
    const float* weight; const float* bias;
    float* out;       int ld_out, off_out;
    void* out_split;  int lds_out;     /* optional split twin of `out` (see pf_conv_desc; 7x7 2 -> C stems only), same
                                        * channel offset (% 8 == 0); `out` may then be NULL */
} pf_direct_desc;
int pf_conv2d_direct_group(const pf_direct_desc* descs, int n, int cin, int cout, int kh, int kw, int relu,
                           int B, int H8, int W8, void* stream);
/* The same with out_split an f16 map (PF_PREC_F16, lds_out units of 64 channels): the 7x7 flow stems' outputs as operands of
 * the fp16 3x3s under mixed_precision (core/prior_raft.py:190, core/update.py:187-191 / :94-95). */
int pf_conv2d_direct_group_f16(const pf_direct_desc* descs, int n, int cin, int cout, int kh, int kw, int relu,
                               int B, int H8, int W8, void* stream);

/* Small-Cin convolution with stride 1|2 from channel-last or NCHW input (the encoders' 7x7/2 3->64
 * stem, core/extractor.py:112,144; same kernel family as pf_conv2d_direct).  Hout/Wout = OUTPUT map;
 * input map = stride x output.  nchw != 0: `in` is [B,cin,Hin,Win] planes (ld_in/off_in ignored). */
int pf_conv2d_small(const float* in, int nchw, int ld_in, int off_in, int cin,
                    const float* weight, const float* bias, float* out, int ld_out, int off_out, int cout,
                    int kh, int kw, int stride, int relu, int B, int Hout, int Wout, void* stream);

/* ---- encoder glue (core/extractor.py) ---------------------------------------------------------- */

/* Second stage of pf_channel_stats on partials some other kernel produced (pf_conv2d with
 * desc.stats_out): partials [B][nblk][C][2] doubles -> scale / shift [B][C]. */
int pf_channel_stats_final(const double* partials, int B, int Np, int C, int nblk, float eps,
                           float* scale, float* shift, void* stream);

/* Per-(image, channel) InstanceNorm statistics of a channel-last map y [B*Np][C] (C <= 256):
 * scale[b][c] = 1/sqrt(var+eps), shift[b][c] = -mean*scale (biased variance).  Deterministic
 * two-stage fp64 reduction; partials: workspace of B*nblk*C*2 doubles. */
int pf_channel_stats(const float* y, int B, int Np, int C, float eps, float* scale, float* shift,
                     double* partials, int nblk, void* stream);

/* out = relu( res' + relu(y*s + t) ), res' = res | res*rs + rt | relu(res*rs + rt) [res_relu != 0: the skip input is itself
 * a normalised + activated raw conv output that was never materialised -- the stem of the encoder] | absent (ResidualBlock
 * tail, core/extractor.py:41-47).  y,res,out channel-last [B*Np][C]; s,t,rs,rt [B][C]. */
int pf_norm_act(const float* y, const float* s, const float* t, const float* res,
                const float* rs, const float* rt, int res_relu, float* out, int B, int Np, int C, void* stream);

/* FlowHead.conv2 (3x3, C->2; core/update.py:10,13-14) fused with coords1 += delta_flow
 * (core/prior_raft.py:193,196).  x: channel-last hidden features [B*N][ld] (C channels at column 0);
 * weight packed [2][9][C] (exact fp32 dot products); coords1 planar, updated in place; delta
 * (optional, may be NULL): channel-last [B*N][ld_delta] copy of delta_flow. */
int pf_flow_head_out(const float* x, int ld, int C, const float* weight, const float* bias,
                     float* coords1, float* delta, int ld_delta, int B, int H8, int W8, void* stream);


/* coords1 += delta (core/prior_raft.py:193,196).  delta: channel-last, 2 channels at column 0. */
int pf_coords_add(float* coords1, const float* delta, int ld, int B, int H8, int W8, void* stream);
/* dst = src + delta: the same update into the next iteration's coordinates (the training loop keeps every iteration's). */
int pf_coords_add_to(const float* src, const float* delta, int ld, float* dst, int B, int H8, int W8, void* stream);

/* upsample_flow (core/prior_raft.py:58-67): convex 8x upsampling of flow = coords1 - coords0.
 * mask: channel-last [B*N][ld] (576 logits, already scaled by 0.25).  out: [B,2,8*H8,8*W8]. */
int pf_upsample_flow(const float* coords1, const float* mask, int ld, float* out,
                     int B, int H8, int W8, void* stream);

/* ---- layout plumbing ------------------------------------------------------------------------ */

/* NCHW channel slice -> channel-last slice, with activation (0 none, 1 relu, 2 tanh)
 * (core/prior_raft.py:136-142 splits/activations of the context features). */
int pf_to_channel_last(const float* in, int c_total, int c_begin, int c, float* out, int ld_out,
                       int off_out, int act, int B, int N, void* stream);

/* 2x2 space-to-depth: NCHW [B,C,H,W] -> channel-last [B*(H/2)*(W/2)][ld_out], column (py*2+px)*C + c.
 * Feeds the encoders' stem (core/extractor.py:122 `conv1 = Conv2d(3, 64, 7, stride=2, padding=3)`),
 * which pf_conv2d then runs as a 4x4 stride-1 convolution over the 12 stacked channels. */
int pf_space_to_depth2(const float* in, int C, float* out, int ld_out, int B, int H, int W, void* stream);

/* ---- evaluation counterpart ---------------------------------------------- */

/* Per-pixel EPE (evaluate.py:265 `torch.sum((flow - flow_gt)**2, dim=0).sqrt()`) and SEPE
 * (core/utils/spherical.py:20-53 `calculate_great_circle_distance`, R = 1; cosine = 0: method 'Haversine', the one
 * evaluate.py uses; cosine = 1: method 'Cosine', arccos of the spherical law of cosines as written at :40-46) of
 * pred vs gt, both NCHW [B,2,H,W].  epe / sd: [B,H,W]; either may be NULL.
 * The haversine is clamped to [0, 1] before asin(sqrt(.)) and the cosine to [-1, 1] before acos(.): fp32 rounding takes them
 * past 1 for antipodal resp. coincident end points (a perfect prediction in the Cosine form), where the reference's fp32
 * spherical.py:80-84 returns NaN -- a deliberate departure, as in pf_fb_check and pf_flow_render: an antipodal or a
 * coincident end point never gives NaN.  The clamp is two comparisons: a NaN input still gives NaN. */
int pf_flow_metrics(const float* pred, const float* gt, float* epe, float* sd, int cosine, int B, int H, int W,
                    void* stream);

/* Region sums of evaluate.py:246-275 (All / Equator / Poles / Center ...): bit r of bits[n] puts
 * pixel n into region r (nregions <= 8).  weight: [N] cos-latitude weights (evaluate.py:208-213
 * `sd_uni`) or NULL.  partials: double [B][nblk][nregions][3] = per pixel-chunk sums of
 * epe, sd, sd*weight; the caller adds the nblk chunks (deterministic two-stage sum). */
int pf_region_sums(const float* epe, const float* sd, const float* weight, const unsigned char* bits,
                   int nregions, double* partials, int nblk, int B, int N, void* stream);

/* ---- training-step counterpart (the network's backward is NOT built) ------- */

/* One term of `uniform_loss.__call__` (train_flow.py:62-71): with m = (valid >= 0.5 && |gt| < max_flow) * weight[n],
 * partials[b][k][0] = sum m (|du|+|dv|) over pixel chunk k; [1..5] = sum epe, n_valid, n(epe<1), n(<3), n(<5)
 * over the valid pixels (the metrics of :73-79, meaningful for the last prediction).  grad (optional):
 * d(i_weight * loss_i)/d pred = i_weight * m * sign(pred - gt).  pred, gt, grad: [B,2,N]; valid [B,N]; weight [N]. */
int pf_seq_loss(const float* pred, const float* gt, const float* valid, const float* weight, float i_weight,
                float max_flow, float* grad, double* partials, int nblk, int B, int N, void* stream);

/* n <= 32 terms of the same `uniform_loss.__call__` (train_flow.py:62-71: the predictions of all iterations of one branch) in ONE
 * launch: term i = pf_seq_loss(preds[i], gt, valid, weight, i_weights[i], max_flow, grads[i], partials + i * B * nblk * 6, ...),
 * bit for bit.  preds / grads / i_weights are HOST arrays of n device pointers / floats (grads, or single entries of it, may be
 * NULL); partials is [n][B][nblk][6].  (Round 6: the training step's loss was 24 launches of ~13 us one behind the other.) */
int pf_seq_loss_batch(const float* const* preds, const float* gt, const float* valid, const float* weight,
                      const float* i_weights, float max_flow, float* const* grads, double* partials, int nblk, int n,
                      int B, int N, void* stream);

/* Self-supervised criterion of one branch (the statement is csrc/pf_selfsup.h): for each of the n <= 32
 * predictions preds[i] [B,2,H,W] (pixels) the photometric term -- image2 [B,3,H,W] (0..255) sampled at p + f with the taps of
 * pf_cycle_warp, against image1, Charbonnier with eps_photo, weighted by weight [H*W] -- and the first-order edge-aware
 * smoothness term (pairs to the right, the seam included, and downwards; Charbonnier with eps_smooth; edges of image1 through
 * exp(-edge_lambda |dI| / 255)), both divided by z = B * sum weight.  mask [B,H,W] bytes or NULL: a non-zero byte leaves the
 * pixel's photometric term out; so does a flow that is not finite or has |u| or |v| >= max_flow, which also drops the pixel's
 * smoothness pairs.  grads[i] (optional) = i_weights[i] * d (w_photo photo_i + w_smooth smooth_i) / d preds[i], every element
 * written.  partials [n][B][nblk][4] fp64 = {photo, smooth, sum of weight over the pixels used, count of left-out flows} per chunk
 * of ceil(H * W / nblk) consecutive pixels; the caller adds the chunks.  preds / grads / i_weights are HOST arrays as in
 * pf_seq_loss_batch.  blocks: workgroups of the launch, 0 = one per (chunk, image); neither the gradients nor the partials depend
 * on it.  PF_ERR_BAD_ARG: a NULL where one is required, an output whose bytes meet those of an input or of another output, a
 * scalar out of range (an eps whose square underflows, a max_flow that is not finite), blocks outside 0..65536.  PF_ERR_BAD_SHAPE: B < 1, H or W < 2, H * W >= 2^30, n outside 1..32, nblk outside 1..4096. */
int pf_selfsup_loss_batch(const float* const* preds, const float* image1, const float* image2, const float* weight,
                          const unsigned char* mask, const float* i_weights, float* const* grads, double* partials, int nblk,
                          int n, int B, int H, int W, float w_photo, float w_smooth, float eps_photo, float eps_smooth,
                          float edge_lambda, float max_flow, float z, int blocks, void* stream);

/* partials[k] = sum of squares of chunk k of x[0..n): the total norm of `clip_grad_norm_` (train_flow.py:137). */
int pf_sum_squares(const float* x, long n, double* partials, int nblk, void* stream);

/* One fused AdamW step over a flat parameter buffer (torch.optim.AdamW as built by train_flow.py:86-88):
 * g*grad_scale (the clip coefficient), decoupled weight decay, bias-corrected update; step counts from 1. */
int pf_adamw_step(float* p, const float* g, float* m, float* v, long n, double lr, float beta1, float beta2,
                  float eps, double weight_decay, int step, float grad_scale, void* stream);
/* The same update with the step-dependent scalars in device memory: hyper[4] = {1 - lr * weight_decay, lr / (1 - beta1^step),
 * sqrt(1 - beta2^step), grad_scale} (rounded from double like pf_adamw_step does).  Every launch argument is then constant
 * over the steps, so the call can sit in a captured HIP graph of the whole training step (train.GraphedTrainStep): the host
 * rewrites hyper[0..2] between replays, a kernel of the graph writes the clip coefficient hyper[3]. */
int pf_adamw_step_dev(float* p, const float* g, float* m, float* v, long n, float beta1, float beta2, float eps,
                      const float* hyper, void* stream);

/* Backward of pf_dccl_combine / pf_dccl_lookup (autograd through DCCL.__call__, core/corr.py:113-144; coords
 * are detached, core/prior_raft.py:171,176): d_corr -> d_raw (rotate-back transposed; d_own = d_corr), then
 * d_own / d_raw -> gradients of the own and the other pyramid (level i: [B*N][H_i*W_i]).  All outputs are
 * ACCUMULATED with fp32 atomics: zero them once per step. */
/* Backward of pf_warp_gcorr (autograd through cycle_bilinear_sampler + groupwise_corr, core/prior_raft.py:173-174,
 * :77-83; coords detached): d_flaw (4 channels at off_d of [B*N][ld_d]) -> d_f1, d_f2 [B*N][C], both ACCUMULATED. */
int pf_warp_gcorr_bwd(const float* f1, const float* f2, const float* coords, int add_grid, const float* d_flaw,
                      int ld_d, int off_d, float* d_f1, float* d_f2, int B, int H8, int W8, int C, void* stream);

/* Backward of pf_upsample_flow (autograd through upsample_flow, core/prior_raft.py:58-67): g [B,2,8*H8,8*W8] ->
 * d_mask [B*N][ld_d] (all 576 logits written; softmax backward) and d_flow [B,2,H8,W8] (= d coords1, ACCUMULATED). */
int pf_upsample_flow_bwd(const float* coords1, const float* mask, int ld, const float* g, float* d_mask, int ld_d,
                         float* d_flow, int B, int H8, int W8, void* stream);

/* ResidualBlock tail of the encoders on the training tape (core/extractor.py:47): out = relu(x + y); and the backward of any
 * ReLU from its forward output: dx = fwd_out > 0 ? g : 0.  n floats, any layout (elementwise). */
int pf_add_relu(const float* x, const float* y, float* out, long n, void* stream);
int pf_relu_mask(const float* g, const float* fwd_out, float* dx, long n, void* stream);

/* nn.BatchNorm2d with frozen statistics (freeze_bn, train_flow.py:107-108: the context encoder in every stage but `chairs`),
 * optionally with the ReLU behind it (core/extractor.py:41-42,144-146), on channel-last rows [rows][C], one launch:
 *   out = [relu]( x*s + t ),  s = gamma * rsqrt(var + eps),  t = beta - mean * s. */
int pf_bn_frozen_fwd(const float* x, const float* gamma, const float* beta, const float* mean, const float* var,
                     float eps, int relu, float* out, long rows, int C, void* stream);
/* Its backward: g_m = relu ? (x*s + t > 0 ? dy : 0) : dy;  dx = s * g_m;  dgamma[c] (+)= sum g_m * (x - mean) * rsqrt(var + eps),
 * dbeta[c] (+)= sum g_m (accumulate != 0: added to what is there -- the parameters' .grad).  Deterministic fp64 sums through
 * `partials` (nblk*C*2 doubles, nblk <= rows).  Three launches. */
int pf_bn_frozen_bwd(const float* dy, const float* x, const float* gamma, const float* beta, const float* mean,
                     const float* var, float eps, int relu, double* partials, int nblk, float* dx,
                     float* dgamma, float* dbeta, int accumulate, long rows, int C, void* stream);

/* Backward of y = act(x * scale[b,c] + shift[b,c]) on channel-last rows [B*Np][C] (the encoders' norm + ReLU,
 * core/extractor.py:112-147; scale / shift as produced by pf_channel_stats or the folded BatchNorm affine).
 * relu != 0: dy is masked where x*scale+shift <= 0.  instance != 0: InstanceNorm backward,
 * dx = scale * (g - mean(g) - xh * mean(g*xh)) with deterministic fp64 sums through `partials` ([B][nblk][C][2]
 * doubles) and `coef` ([B][C][2] floats); instance == 0: fixed statistics (BatchNorm eval), dx = scale * g. */
int pf_norm_bwd(const float* dy, const float* x, const float* scale, const float* shift, int relu, int instance,
                double* partials, int nblk, float* coef, float* dx, int B, int Np, int C, void* stream);

/* SepConvGRU gate backward of one half-step (core/update.py:46-60), channel-last rows with leading dimensions.
 * Stage Q, before the data gradient of convq:  dq_pre = dh'*z*(1-q^2), dz = dh'*q - dh'*h, dh = dh'*(1-z).
 * Stage ZR, after it (d_rh = gradient of r*h, the first C input channels of convq):
 * dzr_pre[:, :C] = dz*(1-z)*z, dzr_pre[:, C:2C] = d_rh*h*(1-r)*r (the [z|r] gradient of the fused conv), dh += d_rh*r. */
int pf_gru_q_bwd(const float* dh_new, int ld_dhn, const float* z, int ld_z, const float* q, int ld_q,
                 const float* h, int ld_h, float* dq_pre, int ld_dq, float* dz, int ld_dz,
                 float* dh, int ld_dh, long rows, int C, void* stream);
int pf_gru_zr_bwd(const float* dz, int ld_dz, const float* d_rh, int ld_drh, const float* z, int ld_z,
                  const float* r, int ld_r, const float* h, int ld_h, float* dzr_pre, int ld_dzr,
                  float* dh, int ld_dh, long rows, int C, void* stream);

/* Gradient of a SepConvGRU's input x = [inp (C) | out (wout) | flows] once both half-steps' data gradients exist
 * (f1, f2: rows with leading dimensions, x's channel order): d_inp[., c] += f1 + f2 for c < C (inp = relu(cnet) feeds every
 * iteration, core/prior_raft.py:196); d_out[., j] = (f1 + f2)[., C + j] where x[., C + j] > 0 else 0 (out = relu(conv),
 * core/update.py:99,200). */
int pf_gru_dx_finish(const float* f1, int ld_f1, const float* f2, int ld_f2, const float* x, int ld_x,
                     float* d_inp, int ld_dinp, float* d_out, int ld_dout, long rows, int C, int wout, void* stream);

/* Backward of build_pyramid (core/corr.py:99-111): level gradients g0..g3 ([B*N][H_i*W_i]) -> the dense volume
 * gradient, written in place into g0 (avg_pool2d backward with floor semantics for odd sizes). */
int pf_pyramid_bwd(float* g0, const float* g1, const float* g2, const float* g3, int B, int H8, int W8, void* stream);
int pf_dccl_combine_bwd(const float* d_corr, int ld_in, const float* g_back, float* d_raw, int ld,
                        int B, int H8, int W8, void* stream);
/* Backward of pf_dccl_lookup (core/corr.py:113-144): the gradients of its two outputs (d_own, d_raw: [B*N][ld] rows, 324 channels)
 * scattered into the two pyramids' level gradients (accumulated).  clear_raw != 0: every d_raw value read is replaced by 0, so
 * the buffer is ready for the next pf_dccl_combine_bwd, which scatters into it (one fill launch per iteration less). */
int pf_dccl_lookup_bwd(const float* coords, const float* g_w2c, const float* d_own, float* d_raw, int ld,
                       float* own0, float* own1, float* own2, float* own3,
                       float* oth0, float* oth1, float* oth2, float* oth3, int B, int H8, int W8, int clear_raw, void* stream);

/* Weight and bias gradient of a stride-1 convolution (what autograd computes for every nn.Conv2d of
 * core/update.py / core/extractor.py in `loss.backward()`, train_flow.py:135):
 *   dw[o][tap][c] += sum_p dy[p][o] * x[p + off(tap)][c],  db[o] += sum_p dy[p][o]
 * x: channel-last, two-segment virtual concat like pf_conv_desc (in0 | in1); dy: channel-last gradient of the
 * conv's pre-activation output; dw: fp32 in the packed weight layout [Cout_pad128][KH*KW][Cin_pad32], db
 * [Cout_pad128] or NULL -- both ACCUMULATED into (zero them first).  3x3, 1x5, 5x1, 1x1; 3-pass bf16 split.
 * Rows >= cout and columns >= c0 + c1 of dw, and db[cout ...], are never written.
 * Split-K promise: the 4 x 32 pixel tiles (per image) are dealt round-robin to
 *   nsplit = min(ceil(512 / (ceil(cout / 128) * ceil(cin_pad / (kh * kw > 5 ? 32 : 64)))), tiles)
 * splits -- at most 512 --, split s owning tiles s, s + nsplit, ...; each split adds its fp32 partial sums with one atomic per
 * element, in arbitrary order (results are not bit-reproducible).
 * PF_ERR_BAD_ARG: a NULL x0 / dy / dw (or x1 with c1 > 0), a slice off + c past its row ld.  PF_ERR_BAD_SHAPE: another kernel
 * shape; cout, c0, c1, an ld or an offset that is not a multiple of 4; c1 > 0 with c0 % 32 != 0; B, H8, W8, c0, cout < 1.
 * The data gradient needs no entry of its own: dx = pf_conv2d(dy, W') with
 * W'[c][o][ky][kx] = W[o][c][KH-1-ky][KW-1-kx]. */
int pf_conv2d_wgrad(const float* x0, int ld0, int off0, int c0, const float* x1, int ld1, int off1, int c1,
                    const float* dy, int ld_dy, int off_dy, int cout, float* dw, float* db,
                    int kh, int kw, int B, int H8, int W8, void* stream);

/* Weight / bias gradient of a small-Cin convolution (the 7x7 stems: core/extractor.py:122 3->64 stride 2,
 * core/update.py:87,173,175 2->128 stride 1; their inputs carry no gradient): exact fp32,
 *   dw[o][c][ky][kx] += sum_p dy[p][o] * x[stride*p + (ky,kx) - pad][c],  db[o] += sum_p dy[p][o]
 * x: NCHW planes (nchw != 0) or a channel-last slice; dy: channel-last [B*Hout*Wout][ld_dy]; dw in the framework's own
 * parameter layout [Cout][Cin][KH][KW]; dw, db ACCUMULATED.  cin <= 4, kh*kw <= 52, stride 1 | 2 (PF_ERR_BAD_SHAPE otherwise,
 * as for cout, ld_dy or off_dy that is not a multiple of 4); PF_ERR_BAD_ARG: a NULL x / dy / dw, a slice past its row, and for
 * the _ws form a NULL workspace or one shorter than pf_conv2d_wgrad_small_ws_floats(...). */
int pf_conv2d_wgrad_small(const float* x, int nchw, int ld_in, int off_in, int cin,
                          const float* dy, int ld_dy, int off_dy, int cout, float* dw, float* db,
                          int kh, int kw, int stride, int B, int Hout, int Wout, void* stream);
/* The same through a caller-provided workspace (pf_conv2d_wgrad_small_ws_floats(...) floats, no initialisation needed; private to
 * the call until it has finished): every workgroup stores its partial sums there and a second launch adds them with 8 atomics per
 * weight.  The form above ends with one atomic per weight per workgroup on the same few hundred cache lines, which was most of its
 * time (414 -> see DESIGN.md section 7 us for the encoder stem at 384x512). */
long pf_conv2d_wgrad_small_ws_floats(int cin, int cout, int kh, int kw, int B, int Hout, int Wout);
int pf_conv2d_wgrad_small_ws(const float* x, int nchw, int ld_in, int off_in, int cin,
                             const float* dy, int ld_dy, int off_dy, int cout, float* dw, float* db,
                             int kh, int kw, int stride, int B, int Hout, int Wout,
                             float* workspace, long workspace_floats, void* stream);

/* channel-last slice -> NCHW. */
int pf_to_nchw(const float* in, int ld_in, int off_in, int c, float* out, int B, int N,
               void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PRIORFLOW_HIP_H */
