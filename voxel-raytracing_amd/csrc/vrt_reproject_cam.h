// vrt_reproject_cam.h -- temporal reprojection for ray cameras (vrt_reproject_camera): where a world point was on the previous
// frame's screen under each of the three vrt_ray_camera models of vrt_raygen.h, and what one pixel of the history becomes.
// THE DEFINITION: compiled for the device by vrt_reproject_cam.hip and for the host by tests/native/reproject_cam_host.cpp; the
// numpy float32 restatement in tests/reproject_cam_reference.py matches it bit for bit.  Only vrt_spec.h operations, every fp32
// step in the written order (-ffp-contract=off).
//
// The history's format, the miss rule (step 1), the taps and their exact surface test (4), the blend (5) and what is written (6)
// are vrt_reproject.h's.  They are RESTATED here, not shared: every factoring of reproject_pixel that was tried (a camera policy
// as a template parameter, with the projection returning through references, as a struct, or calling a continuation) changed the
// machine code of k_reproject -- the mildest one commuted the operands of the two tap-weight multiplications -- and k_reproject
// stays instruction-identical.  What differs from vrt_reproject.h is marked [cam].
//
// For a hit point P and d = P - prev.cam_pos, step 2 is, per model:
//
// VRT_CAMERA_PERSPECTIVE -- vrt_reproject.h's Cramer form over the basis raygen_consts_of builds:
//     U = cam_right * tan_half      V = ((cam_up * tan_half) * H) / W      Cv = normalize(cam_dir) + J
//     R0 = V x Cv, R1 = Cv x U, R2 = U x V, det = U . R0
//     a = d . R0, b = d . R1, l = d . R2;   front: l finite, != 0, of det's sign
//     sx = a / l, sy = b / l;   qx = ((sx + 1) * 0.5) * W - 0.5,  qy = ((sy + 1) * 0.5) * H - 0.5
//   With tan_half == 1.0f every constant equals reproject_consts' bit for bit (x * 1.0f == x), so the whole result equals
//   vrt_reproject's.
//
// VRT_CAMERA_ORTHOGRAPHIC -- the rays are origin = pos + sx U + sy V, dir = cd (no jitter), so with Cv = cd in the same products
//     sx = (d . R0) / det, sy = (d . R1) / det, l = d . R2;   front: l finite, != 0, of det's sign (the previous camera saw only
//     what lies in front of its plane);   qx, qy as above.
//
// VRT_CAMERA_PANORAMA -- skyColor's mapping (frag:98-105), which the panorama's rays invert:
//     u = atan2_spec(d.z, d.x) * 0.1591f + 0.5f        t = asin_spec(-normalize3(d).y) * 0.3183f + 0.5f
//     qx = u * W - 0.5f, qy = t * H - 0.5f;   front: d finite and not all zero.
//   The image is periodic in x -- up to the 0.0022 rad by which 1 / 0.1591 exceeds 2 pi -- so a history tap at column -1 reads
//   column W - 1 and one at column W reads column 0 (u lies in (0, 1), so qx lies in (-0.5, W - 0.5) and no tap is further out);
//   in y taps are clipped as in vrt_reproject.h.  The surface test is exact, so a wrapped tap that shows another surface is dropped
//   like any other.  Motion is the plain difference qx - px, NOT taken the short way round: a surface that crossed the seam has a
//   motion of almost +-W.
//
// The tap tolerance: perspective and panorama tol_abs + tol_rel * |P - cur_pos| (a footprint grows with depth); orthographic
// tol_abs + tol_rel (a parallel view's footprint does not).  The default tol_rel is two pixel footprints: perspective 4 |U| / W per
// unit of depth, orthographic 4 |U| / W voxels, panorama 2 / (0.1591f * W) per unit of depth (a pixel spans 1 / (0.1591 W) rad).
#pragma once

#include "vrt_reproject.h"
#include "vrt_raygen.h"

namespace vrt {

// The pixel-independent part, computed once per call on the host in fp32: vrt_reproject.h's constants and the model.  The
// panorama uses prev_pos, cur_pos, the tolerances and the sizes only (its R0, R1, R2, det are 0).
struct ReprojectCamConsts {
    ReprojectConsts k;
    int32_t         model;
};

// 0: ok; 1: the models differ; 2: the current camera is rejected by raygen_consts_of; 3: the previous camera is; 4: the previous
// camera's basis is degenerate in fp32 (det == 0 or not finite)
inline int reproject_cam_consts(int32_t W, int32_t H, const vrt_ray_camera& cur, const vrt_ray_camera& prev, float tol_abs,
                                float tol_rel, uint32_t max_history, ReprojectCamConsts& c)
{
    RayCamConsts rc, rp;
    if (cur.model != prev.model) return 1;
    if (raygen_consts_of(cur, W, H, rc) != 0) return 2;
    if (raygen_consts_of(prev, W, H, rp) != 0) return 3;
    ReprojectConsts& k = c.k;
    c.model = prev.model;
    k.R0 = k.R1 = k.R2 = mk3(0.0f, 0.0f, 0.0f);
    k.det = 0.0f;
    k.prev_pos = rp.pos; k.cur_pos = rc.pos;
    k.tol_abs = tol_abs; k.tol_rel = tol_rel;
    k.W = rp.Wf; k.H = rp.Hf; k.Wi = W; k.Hi = H;
    k.max_history = max_history;
    if (prev.model == VRT_CAMERA_PANORAMA) return 0;
    // (the perspective model's jitter; 0 for the orthographic one.  cd.z as it is: J.z == 0 is not added, as in reproject_consts)
    const f3 Cv = mk3(rp.cd.x + rp.jx, rp.cd.y + rp.jy, rp.cd.z);
    const f3 Co = prev.model == VRT_CAMERA_PERSPECTIVE ? Cv : rp.cd;
    k.R0 = rp_cross(rp.V, Co); k.R1 = rp_cross(Co, rp.U); k.R2 = rp_cross(rp.U, rp.V);
    k.det = dot3(rp.U, k.R0);
    return rp_finite(k.det) && k.det != 0.0f ? 0 : 4;
}

// default tol_rel: two pixel footprints (0 for a camera raygen_consts_of rejects)
inline float reproject_cam_default_tol_rel(const vrt_ray_camera& cur, int32_t W)
{
    RayCamConsts rc;
    if (W <= 0 || raygen_consts_of(cur, W, 1, rc) != 0) return 0.0f;
    if (cur.model == VRT_CAMERA_PANORAMA) return 2.0f / (0.1591f * (float)W);
    return (4.0f * len3(rc.U)) / (float)W;
}

// Pixel (px, py) under camera model MODEL: P4 its position texel (xyz used), N its normal texel, c its RGBA8 colour.  hs / hc: the
// previous frame's history planes (W x H texels), both nullptr to start a new sequence.  Gathers up to four texels of each.
template <int MODEL>
VRT_HD void reproject_cam_pixel(const ReprojectConsts& k, int px, int py, const rp_u4 P4, uint32_t N, uint32_t c,
                                const rp_u4* hs, const rp_u2* hc, ReprojectPixel& o)
{
    const uint32_t c0 = c & 255u, c1 = (c >> 8) & 255u, c2 = (c >> 16) & 255u, c3 = c >> 24;
    o.mvx = 0.0f; o.mvy = 0.0f;
    if (N == 0u) {                                             // 1. miss
        o.color16.x = (c0 << 8) | (c1 << 24); o.color16.y = (c2 << 8) | (c3 << 24);
        o.surface.x = 0u; o.surface.y = 0u; o.surface.z = 0u; o.surface.w = 1u << 24;
        o.resolved = c;
        return;
    }
    const uint32_t nbits = N & 0xFFFFFFu;
    const f3 P = mk3(rp_u2f(P4.x), rp_u2f(P4.y), rp_u2f(P4.z));
    // 2. project into the previous frame [cam]
    const f3 d = mk3(P.x - k.prev_pos.x, P.y - k.prev_pos.y, P.z - k.prev_pos.z);
    bool front;
    float a = 0.0f, b = 0.0f, l = 0.0f;
    if (MODEL == VRT_CAMERA_PANORAMA) {
        front = rp_finite(d.x) && rp_finite(d.y) && rp_finite(d.z) && !(d.x == 0.0f && d.y == 0.0f && d.z == 0.0f);
    } else {
        a = dot3(d, k.R0); b = dot3(d, k.R1); l = dot3(d, k.R2);
        front = rp_finite(l) && l != 0.0f && ((l > 0.0f) == (k.det > 0.0f));
    }
    uint32_t ws = 0u, s0 = 0u, s1 = 0u, s2 = 0u, s3 = 0u, cmin = 255u;
    if (front) {
        float qx, qy;
        if (MODEL == VRT_CAMERA_PANORAMA) {
            const float u = atan2_spec(d.z, d.x) * 0.1591f + 0.5f;
            const float t = asin_spec(-normalize3(d).y) * 0.3183f + 0.5f;
            qx = u * k.W - 0.5f;
            qy = t * k.H - 0.5f;
        } else {
            const float sx = div_spec(a, MODEL == VRT_CAMERA_ORTHOGRAPHIC ? k.det : l);
            const float sy = div_spec(b, MODEL == VRT_CAMERA_ORTHOGRAPHIC ? k.det : l);
            qx = ((sx + 1.0f) * 0.5f) * k.W - 0.5f;
            qy = ((sy + 1.0f) * 0.5f) * k.H - 0.5f;
        }
        o.mvx = qx - (float)px; o.mvy = qy - (float)py;      // 3. motion, inside the frame or not (the panorama's: not the short way round)
        if (hs != nullptr && rp_finite(qx) && rp_finite(qy)) { // 4. taps and weights
            const float x0f = floorf(qx), y0f = floorf(qy);
            const int wx = (int)floorf((qx - x0f) * 256.0f + 0.5f), wy = (int)floorf((qy - y0f) * 256.0f + 0.5f);
            // (clamped before the conversion: beyond [-1, W - 1] no tap lies inside the frame, however far beyond)
            const int x0 = (int)fminf(fmaxf(x0f, -2.0f), k.W), y0 = (int)fminf(fmaxf(y0f, -2.0f), k.H);
            float tol;                                         // [cam]
            if (MODEL == VRT_CAMERA_ORTHOGRAPHIC) tol = k.tol_abs + k.tol_rel;
            else {
                const f3 dc = mk3(P.x - k.cur_pos.x, P.y - k.cur_pos.y, P.z - k.cur_pos.z);
                tol = k.tol_abs + k.tol_rel * len3(dc);
            }
            const float tol2 = tol * tol;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
            for (int t = 0; t < 4; t++) {
                int tx = x0 + (t & 1);
                const int ty = y0 + (t >> 1);
                // [cam] the panorama is periodic in x: one period; what is still outside (never a panorama's own q) is dropped below
                if (MODEL == VRT_CAMERA_PANORAMA) tx = tx < 0 ? tx + k.Wi : (tx >= k.Wi ? tx - k.Wi : tx);
                const uint32_t w = (uint32_t)((t & 1) ? wx : 256 - wx) * (uint32_t)((t >> 1) ? wy : 256 - wy);
                if (w == 0u || tx < 0 || tx >= k.Wi || ty < 0 || ty >= k.Hi) continue;
                const size_t idx = (size_t)ty * (size_t)k.Wi + (size_t)tx;
#if defined(__HIP_DEVICE_COMPILE__)
                // position, normal and count in ONE 16-byte load (vrt_reproject.h)
                typedef unsigned int rp_v4 __attribute__((ext_vector_type(4)));
                const rp_v4 sv = *reinterpret_cast<const rp_v4*>(hs + idx);
                rp_u4 s; s.x = sv.x; s.y = sv.y; s.z = sv.z; s.w = sv.w;
#else
                const rp_u4 s = hs[idx];
#endif
                if ((s.w & 0xFFFFFFu) != nbits) continue;
                const f3 e = mk3(rp_u2f(s.x) - P.x, rp_u2f(s.y) - P.y, rp_u2f(s.z) - P.z);
                if (!(dot3(e, e) <= tol2)) continue;
                const rp_u2 h = hc[idx];
                ws += w;
                s0 += w * (h.x & 0xFFFFu); s1 += w * (h.x >> 16); s2 += w * (h.y & 0xFFFFu); s3 += w * (h.y >> 16);
                const uint32_t cnt = s.w >> 24;
                cmin = cnt < cmin ? cnt : cmin;
            }
        }
    }
    // 5. blend
    uint32_t n = 1u, o0 = c0 << 8, o1 = c1 << 8, o2 = c2 << 8, o3 = c3 << 8;
    if (ws != 0u) {
        n = cmin + 1u < k.max_history ? cmin + 1u : k.max_history;
        const uint32_t half = ws / 2u, hn = n / 2u;
        o0 = (((s0 + half) / ws) * (n - 1u) + (c0 << 8) + hn) / n;
        o1 = (((s1 + half) / ws) * (n - 1u) + (c1 << 8) + hn) / n;
        o2 = (((s2 + half) / ws) * (n - 1u) + (c2 << 8) + hn) / n;
        o3 = (((s3 + half) / ws) * (n - 1u) + (c3 << 8) + hn) / n;
    }
    // 6. write
    o.color16.x = o0 | (o1 << 16); o.color16.y = o2 | (o3 << 16);
    o.surface.x = P4.x; o.surface.y = P4.y; o.surface.z = P4.z; o.surface.w = nbits | (n << 24);
    const uint32_t r0 = (o0 + 128u) >> 8, r1 = (o1 + 128u) >> 8, r2 = (o2 + 128u) >> 8, r3 = (o3 + 128u) >> 8;
    o.resolved = (r0 < 255u ? r0 : 255u) | ((r1 < 255u ? r1 : 255u) << 8) | ((r2 < 255u ? r2 : 255u) << 16) | ((r3 < 255u ? r3 : 255u) << 24);
}

// the pixel under a model known only at run time (the host loop of the tests)
VRT_HD void reproject_cam_pixel_of(const ReprojectCamConsts& c, int px, int py, const rp_u4 P4, uint32_t N, uint32_t col,
                                   const rp_u4* hs, const rp_u2* hc, ReprojectPixel& o)
{
    if (c.model == VRT_CAMERA_PANORAMA) reproject_cam_pixel<VRT_CAMERA_PANORAMA>(c.k, px, py, P4, N, col, hs, hc, o);
    else if (c.model == VRT_CAMERA_ORTHOGRAPHIC) reproject_cam_pixel<VRT_CAMERA_ORTHOGRAPHIC>(c.k, px, py, P4, N, col, hs, hc, o);
    else reproject_cam_pixel<VRT_CAMERA_PERSPECTIVE>(c.k, px, py, P4, N, col, hs, hc, o);
}

} // namespace vrt
