// Per-pixel functions of the perspective viewports and cube maps (include/priorflow_hip.h:
// pf_viewport_image, pf_viewport_flow, pf_cubemap_to_erp).
//
// Geometry, the reference's convention (core/utils/projection_prim_ortho.py:264-430), stated once for the three kernels:
//   ERP pixel (m, n) of an H x W map:  theta = ((m + 1/2) / W - 1/2) 2 pi,  phi = (1/2 - (n + 1/2) / H) pi,
//                                      s(m, n) = (cos phi cos theta, cos phi sin theta, sin phi)
//   a direction d:                     theta = atan2(d_y, d_x),  phi = asin(d_z / |d|),
//                                      m = (theta / 2 pi + 1/2) W - 1/2,  n = (1/2 - phi / pi) H - 1/2
//   a view (R, f, h, w): R's columns are forward, right, up in world axes, f the focal length in pixels, the principal point
//   (c_x, c_y) = ((w - 1) / 2, (h - 1) / 2); pixel (i, j) has the camera ray (1, (j - c_x) / f, -(i - c_y) / f) and the world ray
//   d = R ray; proj(q) = (c_x + f q_r / q_f, c_y - f q_u / q_f) with (q_f, q_r, q_u) = R^T q.
// The reference's diverge_zero nudge (:69-74) is NOT applied: atan2f is defined on the axes, and a nudge of 1e-6 would move the
// sample position by more than the arithmetic does.  phi is evaluated as atan2(d_z, hypot(d_x, d_y)), the same angle, which keeps
// its fp32 error at a few ulp towards the poles where asin's grows without bound.
// The same functions compile for the host (tests/emu/pf_emu_viewport.cpp).  Built without contraction like every unit.
#pragma once
#include "pf_common.h"
#include "pf_elem.h"
#include "../../include/priorflow_hip.h"      // PF_VIEW_MAX, PF_VIEW_WORDS, PF_VIEW_*; checks the definitions against their declarations

// One row of the view table: R row-major, f, h, w (fp32).
#define PF_VP_ROW 12
#define PF_VP_F 9
#define PF_VP_H 10
#define PF_VP_W 11
static_assert(PF_VP_ROW == PF_VIEW_WORDS, "the row length of pf_viewport.h and of the public header");
#define PF_VP_MAX_GRID_Y 65535

struct PfViewTable { float row[PF_VIEW_MAX][PF_VP_ROW]; };        // passed to the kernels by value: no copy to the device
struct PfVec3 { float x, y, z; };

#define PF_VP_PI 3.14159265358979323846f
#define PF_VP_TWO_PI 6.28318530717958647692f

PF_HD float pf_vp_theta(float m, int W) { return (((m + 0.5f) / (float)W - 0.5f) * 2.f) * PF_VP_PI; }
PF_HD float pf_vp_phi(float n, int H) { return (0.5f - (n + 0.5f) / (float)H) * PF_VP_PI; }
PF_HD PfVec3 pf_vp_dir(float ct, float st, float cp, float sp) { PfVec3 s; s.x = cp * ct; s.y = cp * st; s.z = sp; return s; }
// s(m, n)
PF_HD PfVec3 pf_vp_sphere(float m, float n, int H, int W) {
    const float t = pf_vp_theta(m, W), p = pf_vp_phi(n, H);
    return pf_vp_dir(cosf(t), sinf(t), cosf(p), sinf(p));
}
// the ERP position of a direction (any length)
PF_HD void pf_vp_erp(const PfVec3& d, int H, int W, float& m, float& n) {
    const float theta = atan2f(d.y, d.x);
    const float phi = atan2f(d.z, sqrtf(d.x * d.x + d.y * d.y));
    m = (theta / PF_VP_TWO_PI + 0.5f) * (float)W - 0.5f;
    n = (0.5f - phi / PF_VP_PI) * (float)H - 0.5f;
}
PF_HD float pf_vp_norm(const PfVec3& d) { return sqrtf((d.x * d.x + d.y * d.y) + d.z * d.z); }
// R v and R^T v of a table row
PF_HD PfVec3 pf_vp_rot(const float* R, float a, float b, float c) {
    PfVec3 o;
    o.x = (R[0] * a + R[1] * b) + R[2] * c;
    o.y = (R[3] * a + R[4] * b) + R[5] * c;
    o.z = (R[6] * a + R[7] * b) + R[8] * c;
    return o;
}
PF_HD PfVec3 pf_vp_rot_t(const float* R, const PfVec3& q) {           // (q_f, q_r, q_u)
    PfVec3 o;
    o.x = (R[0] * q.x + R[3] * q.y) + R[6] * q.z;
    o.y = (R[1] * q.x + R[4] * q.y) + R[7] * q.z;
    o.z = (R[2] * q.x + R[5] * q.y) + R[8] * q.z;
    return o;
}
// world ray of pixel (i, j) of a view
PF_HD PfVec3 pf_vp_ray(const float* row, int i, int j, int h, int w) {
    const float f = row[PF_VP_F];
    const float cx = (float)(w - 1) * 0.5f, cy = (float)(h - 1) * 0.5f;
    return pf_vp_rot(row, 1.f, ((float)j - cx) / f, -(((float)i - cy) / f));
}
// proj(q) from camera coordinates (q_f, q_r, q_u)
PF_HD void pf_vp_proj(const PfVec3& c, float f, float cx, float cy, float& x, float& y) {
    x = cx + (f * c.y) / c.x;
    y = cy - (f * c.z) / c.x;
}

// ---- ERP -> views, images ----------------------------------------------------------------------------------------------------
// form PF_VIEW_F32: in [B,C,H,W] fp32 -> out [B,V,C,h,w] fp32; PF_VIEW_U8: in [B,H,W,C] bytes -> out [B,V,h,w,C] bytes, floor(x + 1/2)
// clamped to 0..255.  No anti-aliasing: a view coarser than the panorama is point-sampled (four taps), as grid_sample would.
struct PfViewImageArgs { const void* in; void* out; int B, V, C, H, W, h, w, form; PfViewTable t; };
PF_HD unsigned char pf_vp_byte(float x) {
    const float q = floorf(x + 0.5f);
    return (unsigned char)(q >= 0.f ? (q <= 255.f ? (int)q : 255) : 0);
}
PF_HD void pf_vp_image_pixel(const PfViewImageArgs& a, int bv, int pix) {       // bv = b * V + v, pix = i * w + j
    const int b = bv / a.V, v = bv - b * a.V;
    const int i = pix / a.w, j = pix - i * a.w;
    float m, n;
    pf_vp_erp(pf_vp_ray(a.t.row[v], i, j, a.h, a.w), a.H, a.W, m, n);
    const PfWrapTaps t = pf_wraptaps(m, n, a.H, a.W);         // x wraps, y clamps: a ray towards a pole reads the pole row
    const long N = (long)a.H * a.W, hw = (long)a.h * a.w;
    if (a.form == PF_VIEW_F32) {
        const float* src = static_cast<const float*>(a.in) + (long)b * a.C * N;
        float* dst = static_cast<float*>(a.out) + (long)bv * a.C * hw + pix;
        for (int c = 0; c < a.C; ++c) {
            const float* s = src + c * N;
            dst[c * hw] = pf_wrapmix(t, s[t.ia], s[t.ib], s[t.ic], s[t.id]);
        }
    } else {
        const unsigned char* src = static_cast<const unsigned char*>(a.in) + (long)b * N * a.C;
        unsigned char* dst = static_cast<unsigned char*>(a.out) + ((long)bv * hw + pix) * a.C;
        const long C = a.C;
        for (int c = 0; c < a.C; ++c)
            dst[c] = pf_vp_byte(pf_wrapmix(t, (float)src[t.ia * C + c], (float)src[t.ib * C + c], (float)src[t.ic * C + c],
                                           (float)src[t.id * C + c]));
    }
}

// ---- ERP flow -> pinhole flow ------------------------------------------------------------------------------------------------
// For the pixel's unit ray p^, its ERP position and the four wrap / clamp taps k with weights w_k:
//   s_k = s(m_k, n_k),  e_k = s(m_k + u_k, clamp(n_k + v_k, -1/2, H - 1/2))   (flow2endpoint's rule, :200-218),
//   q = p^ + sum w_k (e_k - s_k),  out = proj(q) - proj(p^), both from pf_vp_proj.
// The 3-D displacement is interpolated, never u or v: the seam needs no un-wrapping and a zero flow gives exactly (0, 0)
// (e_k and s_k come from the same expressions on the same bits).  valid = 1 exactly when the eight flow values of the taps are
// finite and q_f > min_forward |q|; where it is 0 the flow is (0, 0).
struct PfViewFlowArgs { const float* flow; float* out; unsigned char* valid; int B, V, H, W, h, w; float min_forward; PfViewTable t; };
PF_HD void pf_vp_flow_pixel(const PfViewFlowArgs& a, int bv, int pix) {
    const int b = bv / a.V, v = bv - b * a.V;
    const int i = pix / a.w, j = pix - i * a.w;
    const float* row = a.t.row[v];
    const PfVec3 d = pf_vp_ray(row, i, j, a.h, a.w);
    float m, n;
    pf_vp_erp(d, a.H, a.W, m, n);
    const PfWrapTaps t = pf_wraptaps(m, n, a.H, a.W);         // indices inside the map for any bits
    const long N = (long)a.H * a.W, hw = (long)a.h * a.w;
    const float* fu = a.flow + (long)b * 2 * N;
    const float* fv = fu + N;
    const int idx[4] = {t.ia, t.ib, t.ic, t.id};
    float* ou = a.out + (long)bv * 2 * hw + pix;
    unsigned char ok = 1;
    float u[4], w[4];
    for (int k = 0; k < 4; ++k) {
        u[k] = fu[idx[k]]; w[k] = fv[idx[k]];
        if (!(pf_finite(u[k]) && pf_finite(w[k]))) ok = 0;
    }
    float ox = 0.f, oy = 0.f;
    if (ok) {
        const float dn = pf_vp_norm(d);
        PfVec3 p; p.x = d.x / dn; p.y = d.y / dn; p.z = d.z / dn;
        float D[4][3];
        for (int k = 0; k < 4; ++k) {
            const int y = idx[k] / a.W, x = idx[k] - y * a.W;
            const PfVec3 s = pf_vp_sphere((float)x, (float)y, a.H, a.W);
            float ey = (float)y + w[k];
            ey = ey < -0.5f ? -0.5f : (ey > (float)a.H - 0.5f ? (float)a.H - 0.5f : ey);
            const PfVec3 e = pf_vp_sphere((float)x + u[k], ey, a.H, a.W);
            D[k][0] = e.x - s.x; D[k][1] = e.y - s.y; D[k][2] = e.z - s.z;
        }
        PfVec3 q;
        q.x = p.x + pf_wrapmix(t, D[0][0], D[1][0], D[2][0], D[3][0]);
        q.y = p.y + pf_wrapmix(t, D[0][1], D[1][1], D[2][1], D[3][1]);
        q.z = p.z + pf_wrapmix(t, D[0][2], D[1][2], D[2][2], D[3][2]);
        const PfVec3 qc = pf_vp_rot_t(row, q), pc = pf_vp_rot_t(row, p);
        if (qc.x > a.min_forward * pf_vp_norm(q)) {             // (a NaN compares false)
            const float f = row[PF_VP_F], cx = (float)(a.w - 1) * 0.5f, cy = (float)(a.h - 1) * 0.5f;
            float qx, qy, px, py;
            pf_vp_proj(qc, f, cx, cy, qx, qy);
            pf_vp_proj(pc, f, cx, cy, px, py);
            ox = qx - px; oy = qy - py;
        } else {
            ok = 0;
        }
    }
    ou[0] = ox; ou[hw] = oy;
    a.valid[(long)bv * hw + pix] = ok;
}

// ---- cube faces -> ERP -------------------------------------------------------------------------------------------------------
// Faces in the order front, right, back, left, up, down; R's columns [forward, right, up]:
//   front +x +y +z | right +y -x +z | back -x -y +z | left -y +x +z | up +z +y -x | down -z +y +x      (all of determinant +1)
// The face of a direction is the axis with the largest |component|, ties to the earlier face; the entries of R are 0 and +-1,
// so R^T d is a selection.  f = s / 2.  The taps are clamped to the face: no filtering across face edges.
PF_HD PfVec3 pf_vp_cube_cam(const PfVec3& d, int face) {
    PfVec3 c;
    switch (face) {
        case 0: c.x = d.x; c.y = d.y; c.z = d.z; break;
        case 1: c.x = d.y; c.y = -d.x; c.z = d.z; break;
        case 2: c.x = -d.x; c.y = -d.y; c.z = d.z; break;
        case 3: c.x = -d.y; c.y = d.x; c.z = d.z; break;
        case 4: c.x = d.z; c.y = d.y; c.z = -d.x; break;
        default: c.x = -d.z; c.y = d.y; c.z = d.x; break;
    }
    return c;
}
PF_HD int pf_vp_cube_face(const PfVec3& d) {
    const float fwd[6] = {d.x, d.y, -d.x, -d.y, d.z, -d.z};
    int best = 0;
    for (int k = 1; k < 6; ++k) if (fwd[k] > fwd[best]) best = k;
    return best;
}
struct PfCubeErpArgs { const float* faces; float* out; int B, C, s, H, W; };
PF_HD void pf_vp_cube_pixel(const PfCubeErpArgs& a, int b, int pix) {           // pix = n * W + m
    const int n = pix / a.W, m = pix - n * a.W;
    const PfVec3 d = pf_vp_sphere((float)m, (float)n, a.H, a.W);
    const int face = pf_vp_cube_face(d);
    const float c0 = (float)(a.s - 1) * 0.5f;
    float px, py;
    pf_vp_proj(pf_vp_cube_cam(d, face), (float)a.s * 0.5f, c0, c0, px, py);
    float fx = floorf(px), fy = floorf(py);
    const float xw = px - fx, yw = py - fy;
    const float hi = (float)(a.s - 1);
    if (!(fx >= -1.f)) fx = -1.f;                             // inside [-1/2, s - 1/2] by construction; the guards keep every read
    if (!(fx <= hi)) fx = hi;                                 // inside the face whatever the arithmetic gives
    if (!(fy >= -1.f)) fy = -1.f;
    if (!(fy <= hi)) fy = hi;
    const int x0 = (int)fx < 0 ? 0 : (int)fx, y0 = (int)fy < 0 ? 0 : (int)fy;
    const int x1 = (int)fx + 1 > a.s - 1 ? a.s - 1 : (int)fx + 1, y1 = (int)fy + 1 > a.s - 1 ? a.s - 1 : (int)fy + 1;
    PfWrapTaps t;
    t.ia = y0 * a.s + x0; t.ib = y1 * a.s + x0; t.ic = y0 * a.s + x1; t.id = y1 * a.s + x1;
    t.wa = (1.f - xw) * (1.f - yw); t.wb = (1.f - xw) * yw; t.wc = xw * (1.f - yw); t.wd = xw * yw;
    const long ss = (long)a.s * a.s, N = (long)a.H * a.W;
    const float* src = a.faces + ((long)b * 6 + face) * a.C * ss;
    float* dst = a.out + (long)b * a.C * N + pix;
    for (int c = 0; c < a.C; ++c) {
        const float* s = src + c * ss;
        dst[c * N] = pf_wrapmix(t, s[t.ia], s[t.ib], s[t.ic], s[t.id]);
    }
}

// ---- argument checks shared by the device entries and their host emulation ---------------------------------------------------
static inline bool pf_vp_isfinite(float v) { return fabsf(v) <= 3.402823466e38f; }
// fills the table; h, w: the size every row must state
static inline int pf_vp_table(const float* views, int V, PfViewTable& t, int& h, int& w) {
    if (!views) return PF_ERR_BAD_ARG;
    if (V < 1 || V > PF_VIEW_MAX) return PF_ERR_BAD_SHAPE;
    for (int v = 0; v < V; ++v) {
        const float* r = views + (long)v * PF_VP_ROW;
        for (int k = 0; k < 9; ++k) if (!pf_vp_isfinite(r[k])) return PF_ERR_BAD_ARG;
        if (!(pf_vp_isfinite(r[PF_VP_F]) && r[PF_VP_F] > 0.f)) return PF_ERR_BAD_ARG;
        const float fh = r[PF_VP_H], fw = r[PF_VP_W];
        if (!(fh >= 1.f && fw >= 1.f && fh <= 32768.f && fw <= 32768.f) || fh != floorf(fh) || fw != floorf(fw)) return PF_ERR_BAD_SHAPE;
        if (v == 0) { h = (int)fh; w = (int)fw; }
        else if ((int)fh != h || (int)fw != w) return PF_ERR_BAD_SHAPE;
        for (int k = 0; k < PF_VP_ROW; ++k) t.row[v][k] = r[k];
    }
    for (int v = V; v < PF_VIEW_MAX; ++v) for (int k = 0; k < PF_VP_ROW; ++k) t.row[v][k] = 0.f;
    return PF_OK;
}
static inline int pf_vp_sizes(int B, int V, int H, int W, int h, int w) {
    if (B < 1 || H < 1 || W < 1 || (long)H * W >= (1L << 30) || (long)h * w >= (1L << 30)) return PF_ERR_BAD_SHAPE;
    if ((long)B * V > PF_VP_MAX_GRID_Y) return PF_ERR_BAD_SHAPE;
    return PF_OK;
}
static inline int pf_viewport_image_check(const void* in, void* out, const float* views, int V, int B, int C, int H, int W, int form,
                                          PfViewImageArgs& a) {
    if (!in || !out || in == out) return PF_ERR_BAD_ARG;
    if (form != PF_VIEW_F32 && form != PF_VIEW_U8) return PF_ERR_BAD_ARG;
    int rc = pf_vp_table(views, V, a.t, a.h, a.w);
    if (rc != PF_OK) return rc;
    if (C < 1 || C > 4096) return PF_ERR_BAD_SHAPE;
    rc = pf_vp_sizes(B, V, H, W, a.h, a.w);
    if (rc != PF_OK) return rc;
    a.in = in; a.out = out; a.B = B; a.V = V; a.C = C; a.H = H; a.W = W; a.form = form;
    return PF_OK;
}
static inline int pf_viewport_flow_check(const float* flow, const float* views, int V, float* out, unsigned char* valid, int B, int H,
                                         int W, float min_forward, PfViewFlowArgs& a) {
    if (!flow || !out || !valid || flow == out || (const void*)valid == (const void*)out || (const void*)valid == (const void*)flow)
        return PF_ERR_BAD_ARG;
    if (!(min_forward > 0.f && min_forward < 1.f)) return PF_ERR_BAD_ARG;
    int rc = pf_vp_table(views, V, a.t, a.h, a.w);
    if (rc != PF_OK) return rc;
    rc = pf_vp_sizes(B, V, H, W, a.h, a.w);
    if (rc != PF_OK) return rc;
    a.flow = flow; a.out = out; a.valid = valid; a.B = B; a.V = V; a.H = H; a.W = W; a.min_forward = min_forward;
    return PF_OK;
}
static inline int pf_cubemap_to_erp_check(const float* faces, float* out, int B, int C, int s, int H, int W, PfCubeErpArgs& a) {
    if (!faces || !out || faces == out) return PF_ERR_BAD_ARG;
    if (C < 1 || C > 4096 || s < 1 || s > 32768) return PF_ERR_BAD_SHAPE;
    const int rc = pf_vp_sizes(B, 1, H, W, s, s);
    if (rc != PF_OK) return rc;
    a.faces = faces; a.out = out; a.B = B; a.C = C; a.s = s; a.H = H; a.W = W;
    return PF_OK;
}
