// vrt_upsample.h -- temporal upsampling (vrt_upsample): what one pixel of a DISPLAY-resolution history becomes from one jittered
// render-resolution frame.  THE DEFINITION: compiled for the device by vrt_upsample.hip and for the host by
// tests/native/upsample_host.cpp; the numpy float32 restatement in tests/upsample_reference.py matches it bit for bit.  Only
// vrt_spec.h operations, every fp32 step in the written order (-ffp-contract=off).
//
// The frame is w x h, the history and every output TW x TH (TW >= w, TH >= h).  The jitter sequence of UpscalerStage::update has
// 8 (TW / w)^2 phases so that the samples of consecutive frames land between each other on the display grid; this pass puts each
// sample where it fell.  The reference adds cameraJitter to the ray in WORLD x / y (voxel_volume.frag:319), so a jittered sample is
// not "pixel centre + jitter": its hit point is projected through the UNJITTERED current camera instead, which tells where on the
// display grid it lies for any orientation.  The same projection through the unjittered previous camera tells where the surface
// was; the difference is the motion, and a camera at rest gives exactly 0 because both are the same arithmetic.
// A pixel no sample of this frame fell on (weight 0) carries its history on: blended with weight 0 where the far sample it was given
// shows the history's surface, copied whole from the nearest history texel where it shows another.
//
// The history format, the tap test and the types are vrt_reproject.h's; the tap loop is restated here, not shared, so that
// k_reproject's machine code does not depend on this file.
#pragma once

#include "vrt_reproject.h"

namespace vrt {

// One unjittered camera on the display grid: the ray through screen position (sx, sy) is C + sx U + sy V with U = camRight,
// V = camUp * h / w (the RENDER frame's aspect) and C = normalize(camDir); R0, R1, R2, det as ReprojectConsts states them.
struct UpsampleCamera {
    f3    R0, R1, R2, pos;
    float det;
};

struct UpsampleConsts {
    UpsampleCamera cur, prev;
    float    tol_abs, tol_rel;
    float    TW, TH;
    int32_t  TWi, THi, wi, hi;
    uint32_t max_history;
};

// false: the camera's basis is degenerate (det == 0 or not finite)
inline bool upsample_camera(int32_t w, int32_t h, const float pos[3], const float dir[3], const float right[3], const float up[3],
                            UpsampleCamera& k)
{
    const float fw = (float)w, fh = (float)h;
    const f3 Cv = normalize3(mk3(dir[0], dir[1], dir[2]));
    const f3 U = mk3(right[0], right[1], right[2]);
    const f3 V = mk3((up[0] * fh) / fw, (up[1] * fh) / fw, (up[2] * fh) / fw);
    k.R0 = rp_cross(V, Cv); k.R1 = rp_cross(Cv, U); k.R2 = rp_cross(U, V);
    k.det = dot3(U, k.R0);
    k.pos = mk3(pos[0], pos[1], pos[2]);
    return rp_finite(k.det) && k.det != 0.0f;
}

// 0: fine; 1 / 2: the current / previous camera's basis is degenerate
inline int upsample_consts(int32_t w, int32_t h, int32_t TW, int32_t TH, const float cur_pos[3], const float cur_dir[3],
                           const float cur_right[3], const float cur_up[3], const float prev_pos[3], const float prev_dir[3],
                           const float prev_right[3], const float prev_up[3], float tol_abs, float tol_rel, uint32_t max_history,
                           UpsampleConsts& k)
{
    k.tol_abs = tol_abs; k.tol_rel = tol_rel;
    k.TW = (float)TW; k.TH = (float)TH; k.TWi = TW; k.THi = TH; k.wi = w; k.hi = h;
    k.max_history = max_history;
    if (!upsample_camera(w, h, cur_pos, cur_dir, cur_right, cur_up, k.cur)) return 1;
    if (!upsample_camera(w, h, prev_pos, prev_dir, prev_right, prev_up, k.prev)) return 2;
    return 0;
}

// 1. the render pixel whose footprint holds the centre of display pixel (X, Y)
VRT_HD void upsample_source(const UpsampleConsts& k, int X, int Y, int& rx, int& ry)
{
    const uint32_t x = ((2u * (uint32_t)X + 1u) * (uint32_t)k.wi) / (2u * (uint32_t)k.TWi);
    const uint32_t y = ((2u * (uint32_t)Y + 1u) * (uint32_t)k.hi) / (2u * (uint32_t)k.THi);
    rx = x < (uint32_t)k.wi - 1u ? (int)x : k.wi - 1;
    ry = y < (uint32_t)k.hi - 1u ? (int)y : k.hi - 1;
}

// P through camera c to display-pixel coordinates; false: P is not in front of the camera (x, y untouched)
VRT_HD bool upsample_project(const UpsampleCamera& c, float TW, float TH, f3 P, float& x, float& y)
{
    const f3 d = mk3(P.x - c.pos.x, P.y - c.pos.y, P.z - c.pos.z);
    const float a = dot3(d, c.R0), b = dot3(d, c.R1), l = dot3(d, c.R2);
    if (!(rp_finite(l) && l != 0.0f && ((l > 0.0f) == (c.det > 0.0f)))) return false;
    const float sx = div_spec(a, l), sy = div_spec(b, l);
    x = ((sx + 1.0f) * 0.5f) * TW - 0.5f;
    y = ((sy + 1.0f) * 0.5f) * TH - 0.5f;
    return true;
}

// 3. the weight of a sample that fell at (ux, uy) for display pixel (X, Y), in 1/256: a tent of radius one display pixel in the
// maximum norm.  NaN in either coordinate gives 0 (fmaxf alone would drop a NaN operand, hence the two comparisons).
VRT_HD uint32_t upsample_alpha(float ux, float uy, float X, float Y)
{
    const float dx = fabsf(ux - X), dy = fabsf(uy - Y);
    const float m = fmaxf(dx, dy);
    return (dx < 1.0f && dy < 1.0f) ? (uint32_t)(256 - (int)floorf(m * 256.0f)) : 0u;
}

// 6. the blend of history h (8.8) and colour code c with sample weight a (0..256) at count n (1..255).  The numerator is at most
// 65535 * 65280 + 32640 < 2^32.
VRT_HD uint32_t upsample_blend(uint32_t h, uint32_t c, uint32_t a, uint32_t n)
{
    return (h * (256u * n - a) + (c << 8) * a + 128u * n) / (256u * n);
}

// Display pixel (X, Y): P4 / N / c the position, normal and RGBA8 texels of ITS render pixel (upsample_source).  hs / hc: the
// previous history (TW x TH texels), both nullptr to start a new sequence.  Gathers up to four texels of each.
VRT_HD void upsample_pixel(const UpsampleConsts& k, int X, int Y, const rp_u4 P4, uint32_t N, uint32_t c,
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
    // 3. where the sample fell
    float ux = fX, uy = fY;
    uint32_t alpha = 256u;
    if (upsample_project(k.cur, k.TW, k.TH, P, ux, uy)) alpha = upsample_alpha(ux, uy, fX, fY);
    // 4. where the pixel was
    float vx = 0.0f, vy = 0.0f;
    uint32_t ws = 0u, s0 = 0u, s1 = 0u, s2 = 0u, s3 = 0u, cmin = 255u;
    int nx = -1, ny = -1;                                      // the texel nearest to q, if taps were looked at
    if (upsample_project(k.prev, k.TW, k.TH, P, vx, vy)) {
        o.mvx = vx - ux; o.mvy = vy - uy;
        const float qx = fX + o.mvx, qy = fY + o.mvy;
        if (hs != nullptr && rp_finite(qx) && rp_finite(qy)) { // 5. taps and weights
            const float x0f = floorf(qx), y0f = floorf(qy);
            const int wx = (int)floorf((qx - x0f) * 256.0f + 0.5f), wy = (int)floorf((qy - y0f) * 256.0f + 0.5f);
            const int x0 = (int)fminf(fmaxf(x0f, -2.0f), k.TW), y0 = (int)fminf(fmaxf(y0f, -2.0f), k.TH);
            nx = x0 + (wx >= 128 ? 1 : 0); ny = y0 + (wy >= 128 ? 1 : 0);
            const f3 dc = mk3(P.x - k.cur.pos.x, P.y - k.cur.pos.y, P.z - k.cur.pos.z);
            const float tol = k.tol_abs + k.tol_rel * len3(dc);
            const float tol2 = tol * tol;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
            for (int t = 0; t < 4; t++) {
                const int tx = x0 + (t & 1), ty = y0 + (t >> 1);
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
        // No sample of this frame fell on the pixel, and the far sample it was given shows another surface than its history: the
        // sample says nothing about this pixel, so it carries the history texel nearest to where it was, whole -- colour, surface
        // and count.  (Dropping the history here made a fifth of the pixels of a view full of edges restart every frame from
        // samples that fell elsewhere: tests/test_upsample_cpu.py, the convergence test.)
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

} // namespace vrt
