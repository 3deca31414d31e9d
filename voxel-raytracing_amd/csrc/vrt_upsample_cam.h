// vrt_upsample_cam.h -- temporal upsampling for ray cameras (vrt_upsample_camera): what one pixel of a DISPLAY-resolution history
// becomes from one render-resolution frame drawn through a vrt_ray_camera whose samples were offset within their pixels
// (vrt_camera_rays_offset; the perspective model's camera_jitter does the same).  THE DEFINITION: compiled for the device by
// vrt_upsample_cam.hip and for the host by tests/native/upsample_cam_host.cpp; the numpy float32 restatement in
// tests/upsample_cam_reference.py matches it bit for bit.  Only vrt_spec.h operations, every fp32 step in the written order
// (-ffp-contract=off).
//
// It is vrt_upsample.h's upsample_pixel RESTATED, not shared and not templated into it, for the reason vrt_reproject_cam.h gives:
// every factoring that was tried changed k_reproject's machine code, and k_upsample stays instruction-identical as well.  The
// constants' layout (UpsampleConsts), upsample_source and upsample_blend are vrt_upsample.h's own and are used as they are.  What
// differs from upsample_pixel is marked [cam].
//
// Both projections run through the camera WITHOUT sample offset and WITHOUT jitter, onto the TW x TH grid.  For a hit point P and
// d = P - cam_pos, per model:
//
// VRT_CAMERA_PERSPECTIVE -- vrt_upsample.h's Cramer form over raygen_consts_of(cam, w, h)'s U, V, cd (no J):
//     U = cam_right * tan_half      V = ((cam_up * tan_half) * h) / w      Cv = normalize(cam_dir)
//     R0 = V x Cv, R1 = Cv x U, R2 = U x V, det = U . R0
//     a = d . R0, b = d . R1, l = d . R2;   front: l finite, != 0, of det's sign;   sx = a / l, sy = b / l
//   With tan_half == 1.0f every constant equals upsample_camera's bit for bit (x * 1.0f == x), so every plane equals vrt_upsample's.
// VRT_CAMERA_ORTHOGRAPHIC -- the same products with U, V scaled by half_width:
//     sx = (d . R0) / det, sy = (d . R1) / det, l = d . R2;   front: l finite, != 0, of det's sign
// both:  x = ((sx + 1) * 0.5) * TW - 0.5,  y = ((sy + 1) * 0.5) * TH - 0.5   (vrt_upsample's screen-to-display step)
// VRT_CAMERA_PANORAMA -- skyColor's mapping (frag:98-105), which the panorama's rays invert:
//     u = atan2_spec(d.z, d.x) * 0.1591f + 0.5f        t = asin_spec(-normalize3(d).y) * 0.3183f + 0.5f
//     x = u * TW - 0.5f, y = t * TH - 0.5f;   front: d finite and not all zero.
//
// The seam (panorama only): the image is periodic in x over TW display pixels.
//   S1. tent: the x distance of a sample at ux from display column X is dx = |ux - X|, then dx = min(dx, TW - dx): a sample of
//       render column 0 pushed left by its offset falls near column TW - 1 and still counts for display column 0.
//   S2. motion stays the plain difference v - u, NOT taken the short way round (as vrt_reproject_camera's).
//   S3. the fetch position qx = X + mvx is brought back by one period into [-0.5, TW - 0.5): + TW if below, - TW if at or above
//       (u, v lie in (-0.5, TW - 0.5), so X + (v - u) lies in (-TW, 2 TW - 1): one period is enough).
//   S4. the tap columns and the carry step's nearest texel wrap by one period, as reproject_cam_pixel<PANORAMA> wraps its taps;
//       rows are clipped.
//
// The tap tolerance: perspective and panorama tol_abs + tol_rel * |P - cur.pos|, orthographic tol_abs + tol_rel
// (vrt_reproject_cam.h); the default tol_rel is reproject_cam_default_tol_rel(cur, w) at the RENDER width: two render-pixel
// footprints, as vrt_upsample has it.
#pragma once

#include "vrt_upsample.h"
#include "vrt_reproject_cam.h"

namespace vrt {

// The pixel-independent part, computed once per call on the host in fp32: vrt_upsample.h's constants and the model.  The panorama
// uses the two positions, the tolerances and the sizes only (its R0, R1, R2, det are 0).
struct UpsampleCamConsts {
    UpsampleConsts k;
    int32_t        model;
};

// false: the basis is degenerate in fp32 (det == 0 or not finite).  rc: raygen_consts_of(cam, w, h)'s constants; J is not used
inline bool upsample_cam_camera(const RayCamConsts& rc, UpsampleCamera& c)
{
    c.R0 = c.R1 = c.R2 = mk3(0.0f, 0.0f, 0.0f);
    c.det = 0.0f;
    c.pos = rc.pos;
    if (rc.model == VRT_CAMERA_PANORAMA) return true;
    c.R0 = rp_cross(rc.V, rc.cd); c.R1 = rp_cross(rc.cd, rc.U); c.R2 = rp_cross(rc.U, rc.V);
    c.det = dot3(rc.U, c.R0);
    return rp_finite(c.det) && c.det != 0.0f;
}

// 0: ok; 1: the models differ; 2 / 3: the current / previous camera is rejected by raygen_consts_of(cam, w, h); 4 / 5: the current /
// previous camera's basis is degenerate in fp32
inline int upsample_cam_consts(int32_t w, int32_t h, int32_t TW, int32_t TH, const vrt_ray_camera& cur, const vrt_ray_camera& prev,
                               float tol_abs, float tol_rel, uint32_t max_history, UpsampleCamConsts& c)
{
    RayCamConsts rc, rp;
    if (cur.model != prev.model) return 1;
    if (raygen_consts_of(cur, w, h, rc) != 0) return 2;
    if (raygen_consts_of(prev, w, h, rp) != 0) return 3;
    UpsampleConsts& k = c.k;
    c.model = cur.model;
    k.tol_abs = tol_abs; k.tol_rel = tol_rel;
    k.TW = (float)TW; k.TH = (float)TH; k.TWi = TW; k.THi = TH; k.wi = w; k.hi = h;
    k.max_history = max_history;
    if (!upsample_cam_camera(rc, k.cur)) return 4;
    if (!upsample_cam_camera(rp, k.prev)) return 5;
    return 0;
}

// [cam] P through camera c to display-pixel coordinates; false: P is not in front of the camera (x, y untouched)
template <int MODEL>
VRT_HD bool upsample_cam_project(const UpsampleCamera& c, float TW, float TH, f3 P, float& x, float& y)
{
    const f3 d = mk3(P.x - c.pos.x, P.y - c.pos.y, P.z - c.pos.z);
    if (MODEL == VRT_CAMERA_PANORAMA) {
        if (!(rp_finite(d.x) && rp_finite(d.y) && rp_finite(d.z) && !(d.x == 0.0f && d.y == 0.0f && d.z == 0.0f))) return false;
        const float u = atan2_spec(d.z, d.x) * 0.1591f + 0.5f;
        const float t = asin_spec(-normalize3(d).y) * 0.3183f + 0.5f;
        x = u * TW - 0.5f;
        y = t * TH - 0.5f;
        return true;
    }
    const float a = dot3(d, c.R0), b = dot3(d, c.R1), l = dot3(d, c.R2);
    if (!(rp_finite(l) && l != 0.0f && ((l > 0.0f) == (c.det > 0.0f)))) return false;
    const float sx = div_spec(a, MODEL == VRT_CAMERA_ORTHOGRAPHIC ? c.det : l);
    const float sy = div_spec(b, MODEL == VRT_CAMERA_ORTHOGRAPHIC ? c.det : l);
    x = ((sx + 1.0f) * 0.5f) * TW - 0.5f;
    y = ((sy + 1.0f) * 0.5f) * TH - 0.5f;
    return true;
}

// 3. upsample_alpha with the panorama's periodic x distance [cam, S1]
template <int MODEL>
VRT_HD uint32_t upsample_cam_alpha(float ux, float uy, float X, float Y, float TW)
{
    float dx = fabsf(ux - X);
    const float dy = fabsf(uy - Y);
    if (MODEL == VRT_CAMERA_PANORAMA) dx = fminf(dx, TW - dx);
    const float m = fmaxf(dx, dy);
    return (dx < 1.0f && dy < 1.0f) ? (uint32_t)(256 - (int)floorf(m * 256.0f)) : 0u;
}

// [cam, S4] a column of the panorama brought back by one period; what is still outside is dropped or clipped by the caller
template <int MODEL>
VRT_HD int upsample_cam_wrap(int tx, int TWi)
{
    if (MODEL == VRT_CAMERA_PANORAMA) return tx < 0 ? tx + TWi : (tx >= TWi ? tx - TWi : tx);
    return tx;
}

// Display pixel (X, Y) under camera model MODEL: P4 / N / c the position, normal and RGBA8 texels of ITS render pixel
// (upsample_source).  hs / hc: the previous history (TW x TH texels), both nullptr to start a new sequence.  Gathers up to four
// texels of each.
template <int MODEL>
VRT_HD void upsample_cam_pixel(const UpsampleConsts& k, int X, int Y, const rp_u4 P4, uint32_t N, uint32_t c,
                               const rp_u4* hs, const rp_u2* hc, ReprojectPixel& o)
{
    const uint32_t c0 = c & 255u, c1 = (c >> 8) & 255u, c2 = (c >> 16) & 255u, c3 = c >> 24;
    o.mvx = 0.0f; o.mvy = 0.0f;
    if (N == 0u) {                                             // 2. miss
        o.color16.x = (c0 << 8) | (c1 << 24); o.color16.y = (c2 << 8) | (c3 << 24);
        o.surface.x = 0u; o.surface.y = 0u; o.surface.z = 0u; o.surface.w = 1u << 24;
        o.resolved = c;
        return;
    }
    const uint32_t nbits = N & 0xFFFFFFu;
    const f3 P = mk3(rp_u2f(P4.x), rp_u2f(P4.y), rp_u2f(P4.z));
    const float fX = (float)X, fY = (float)Y;
    // 3. where the sample fell [cam: the projection, S1]
    float ux = fX, uy = fY;
    uint32_t alpha = 256u;
    if (upsample_cam_project<MODEL>(k.cur, k.TW, k.TH, P, ux, uy)) alpha = upsample_cam_alpha<MODEL>(ux, uy, fX, fY, k.TW);
    // 4. where the pixel was [cam: the projection, S2, S3]
    float vx = 0.0f, vy = 0.0f;
    uint32_t ws = 0u, s0 = 0u, s1 = 0u, s2 = 0u, s3 = 0u, cmin = 255u;
    int nx = -1, ny = -1;                                      // the texel nearest to q, if taps were looked at
    if (upsample_cam_project<MODEL>(k.prev, k.TW, k.TH, P, vx, vy)) {
        o.mvx = vx - ux; o.mvy = vy - uy;
        float qx = fX + o.mvx;
        const float qy = fY + o.mvy;
        if (MODEL == VRT_CAMERA_PANORAMA) qx = qx < -0.5f ? qx + k.TW : (qx >= k.TW - 0.5f ? qx - k.TW : qx);
        if (hs != nullptr && rp_finite(qx) && rp_finite(qy)) { // 5. taps and weights
            const float x0f = floorf(qx), y0f = floorf(qy);
            const int wx = (int)floorf((qx - x0f) * 256.0f + 0.5f), wy = (int)floorf((qy - y0f) * 256.0f + 0.5f);
            const int x0 = (int)fminf(fmaxf(x0f, -2.0f), k.TW), y0 = (int)fminf(fmaxf(y0f, -2.0f), k.TH);
            nx = upsample_cam_wrap<MODEL>(x0 + (wx >= 128 ? 1 : 0), k.TWi); ny = y0 + (wy >= 128 ? 1 : 0);   // [cam, S4]
            float tol;                                         // [cam]
            if (MODEL == VRT_CAMERA_ORTHOGRAPHIC) tol = k.tol_abs + k.tol_rel;
            else {
                const f3 dc = mk3(P.x - k.cur.pos.x, P.y - k.cur.pos.y, P.z - k.cur.pos.z);
                tol = k.tol_abs + k.tol_rel * len3(dc);
            }
            const float tol2 = tol * tol;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
            for (int t = 0; t < 4; t++) {
                const int tx = upsample_cam_wrap<MODEL>(x0 + (t & 1), k.TWi), ty = y0 + (t >> 1);             // [cam, S4]
                const uint32_t w = (uint32_t)((t & 1) ? wx : 256 - wx) * (uint32_t)((t >> 1) ? wy : 256 - wy);
                if (w == 0u || tx < 0 || tx >= k.TWi || ty < 0 || ty >= k.THi) continue;
                const size_t idx = (size_t)ty * (size_t)k.TWi + (size_t)tx;
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
    // 6. blend
    if (ws == 0u && alpha == 0u && nx >= 0 && nx < k.TWi && ny >= 0 && ny < k.THi) {
        // No sample of this frame fell on the pixel, and the far sample it was given shows another surface than its history: it
        // carries the history texel nearest to where it was, whole -- colour, surface and count (vrt_upsample.h)
        const size_t idx = (size_t)ny * (size_t)k.TWi + (size_t)nx;
#if defined(__HIP_DEVICE_COMPILE__)
        typedef unsigned int rp_v4 __attribute__((ext_vector_type(4)));
        const rp_v4 sv = *reinterpret_cast<const rp_v4*>(hs + idx);
        o.surface.x = sv.x; o.surface.y = sv.y; o.surface.z = sv.z; o.surface.w = sv.w;
#else
        o.surface = hs[idx];
#endif
        o.color16 = hc[idx];
        const uint32_t h0 = o.color16.x & 0xFFFFu, h1 = o.color16.x >> 16, h2 = o.color16.y & 0xFFFFu, h3 = o.color16.y >> 16;
        const uint32_t q0 = (h0 + 128u) >> 8, q1 = (h1 + 128u) >> 8, q2 = (h2 + 128u) >> 8, q3 = (h3 + 128u) >> 8;
        o.resolved = (q0 < 255u ? q0 : 255u) | ((q1 < 255u ? q1 : 255u) << 8) | ((q2 < 255u ? q2 : 255u) << 16) | ((q3 < 255u ? q3 : 255u) << 24);
        return;
    }
    uint32_t n = 1u, o0 = c0 << 8, o1 = c1 << 8, o2 = c2 << 8, o3 = c3 << 8;
    if (ws != 0u) {
        n = cmin + 1u < k.max_history ? cmin + 1u : k.max_history;
        const uint32_t half = ws / 2u;
        o0 = upsample_blend((s0 + half) / ws, c0, alpha, n);
        o1 = upsample_blend((s1 + half) / ws, c1, alpha, n);
        o2 = upsample_blend((s2 + half) / ws, c2, alpha, n);
        o3 = upsample_blend((s3 + half) / ws, c3, alpha, n);
    }
    // 7. write
    o.color16.x = o0 | (o1 << 16); o.color16.y = o2 | (o3 << 16);
    o.surface.x = P4.x; o.surface.y = P4.y; o.surface.z = P4.z; o.surface.w = nbits | (n << 24);
    const uint32_t r0 = (o0 + 128u) >> 8, r1 = (o1 + 128u) >> 8, r2 = (o2 + 128u) >> 8, r3 = (o3 + 128u) >> 8;
    o.resolved = (r0 < 255u ? r0 : 255u) | ((r1 < 255u ? r1 : 255u) << 8) | ((r2 < 255u ? r2 : 255u) << 16) | ((r3 < 255u ? r3 : 255u) << 24);
}

// the pixel under a model known only at run time (the host loop of the tests)
VRT_HD void upsample_cam_pixel_of(const UpsampleCamConsts& c, int X, int Y, const rp_u4 P4, uint32_t N, uint32_t col,
                                  const rp_u4* hs, const rp_u2* hc, ReprojectPixel& o)
{
    if (c.model == VRT_CAMERA_PANORAMA) upsample_cam_pixel<VRT_CAMERA_PANORAMA>(c.k, X, Y, P4, N, col, hs, hc, o);
    else if (c.model == VRT_CAMERA_ORTHOGRAPHIC) upsample_cam_pixel<VRT_CAMERA_ORTHOGRAPHIC>(c.k, X, Y, P4, N, col, hs, hc, o);
    else upsample_cam_pixel<VRT_CAMERA_PERSPECTIVE>(c.k, X, Y, P4, N, col, hs, hc, o);
}

} // namespace vrt
