// vrt_reproject.h -- temporal reprojection (vrt_reproject): what one pixel of the history becomes under a moving camera.
// THE DEFINITION: compiled for the device by vrt_reproject.hip and for the host by tests/native/reproject_host.cpp; the
// numpy float32 restatement in tests/reproject_reference.py matches it bit for bit.  Only vrt_spec.h operations, every fp32
// step in the written order (-ffp-contract=off).
//
// The reference leaves this open (voxel_volume.frag:332, "TODO use inverse of camera matrix to reproject old position and
// calculate motion vectors"; its motion target is always 0).  The position plane holds the world-space hit point and a voxel
// normal is one of a few discrete codes, so whether a history texel shows the same surface is tested exactly, not guessed.
//
// History of a pixel (two planes):
//   color16  4 x uint16: the accumulated colour in 8.8 fixed point, all four channels alike
//   surface  4 x 32 bit: xyz = the world position the pixel shows, w = normal8.xyz | count << 24 (count: frames accumulated,
//            1..255; a miss pixel: position 0, normal bits 0)
#pragma once

#include "vrt_spec.h"

namespace vrt {

struct alignas(16) rp_u4 { uint32_t x, y, z, w; };
struct alignas(8)  rp_u2 { uint32_t x, y; };

VRT_HD float    rp_u2f(uint32_t u) { union { uint32_t u; float f; } c; c.u = u; return c.f; }
VRT_HD bool     rp_finite(float x) { return fabsf(x) < INFINITY; }           // false for NaN
VRT_HD f3       rp_cross(f3 a, f3 b) { return mk3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }

// The pixel-independent part, computed once per call on the host in fp32.
// The previous frame's ray through screen position (sx, sy) is C + sx U + sy V (voxel_volume.frag:312-319 as
// raygen_consts / primary_v state it: U = camRight, V = camUp * H / W, C = normalize(camDir) + jitter), so a point
// cam + t (C + sx U + sy V) has, by Cramer's rule with R0 = V x C, R1 = C x U, R2 = U x V and det = U . R0,
//   d . R0 = t sx det,   d . R1 = t sy det,   d . R2 = t det        (d = point - cam)
// and sx, sy are two quotients in which the determinant cancels; t > 0 iff d . R2 has the sign of det.
struct ReprojectConsts {
    f3       R0, R1, R2;
    f3       prev_pos, cur_pos;
    float    det;
    float    tol_abs, tol_rel;
    float    W, H;
    int32_t  Wi, Hi;
    uint32_t max_history;
};

// false: the previous camera's basis is degenerate (det == 0 or not finite)
inline bool reproject_consts(int32_t W, int32_t H, const float prev_pos[3], const float prev_dir[3], const float prev_right[3],
                             const float prev_up[3], const float prev_jitter[2], const float cur_pos[3], float tol_abs,
                             float tol_rel, uint32_t max_history, ReprojectConsts& k)
{
    const float fW = (float)W, fH = (float)H;
    const f3 cd = normalize3(mk3(prev_dir[0], prev_dir[1], prev_dir[2]));
    const f3 U = mk3(prev_right[0], prev_right[1], prev_right[2]);
    const f3 V = mk3((prev_up[0] * fH) / fW, (prev_up[1] * fH) / fW, (prev_up[2] * fH) / fW);
    const float jx = (prev_jitter[0] / fW) * -2.0f, jy = (prev_jitter[1] / fH) * 2.0f;
    const f3 Cv = mk3(cd.x + jx, cd.y + jy, cd.z);
    k.R0 = rp_cross(V, Cv); k.R1 = rp_cross(Cv, U); k.R2 = rp_cross(U, V);
    k.det = dot3(U, k.R0);
    k.prev_pos = mk3(prev_pos[0], prev_pos[1], prev_pos[2]);
    k.cur_pos = mk3(cur_pos[0], cur_pos[1], cur_pos[2]);
    k.tol_abs = tol_abs; k.tol_rel = tol_rel;
    k.W = fW; k.H = fH; k.Wi = W; k.Hi = H;
    k.max_history = max_history;
    return rp_finite(k.det) && k.det != 0.0f;
}

// default tol_rel: two pixel footprints per unit of depth (a pixel is 2 |camRight| / W wide at depth 1)
inline float reproject_default_tol_rel(const float cur_right[3], int32_t W)
{
    return (4.0f * len3(mk3(cur_right[0], cur_right[1], cur_right[2]))) / (float)W;
}

struct ReprojectPixel {
    rp_u2    color16;       // r | g << 16, b | a << 16
    rp_u4    surface;
    uint32_t resolved;      // RGBA8
    float    mvx, mvy;      // where the pixel's surface was on the previous screen, minus where it is: pixels
};

// Pixel (px, py): P4 its position texel (xyz used), N its normal texel, c its RGBA8 colour.  hs / hc: the previous frame's
// history planes (W x H texels), both nullptr to start a new sequence.  Gathers up to four texels of each.
VRT_HD void reproject_pixel(const ReprojectConsts& k, int px, int py, const rp_u4 P4, uint32_t N, uint32_t c,
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
    // 2. project into the previous frame
    const f3 d = mk3(P.x - k.prev_pos.x, P.y - k.prev_pos.y, P.z - k.prev_pos.z);
    const float a = dot3(d, k.R0), b = dot3(d, k.R1), l = dot3(d, k.R2);
    const bool front = rp_finite(l) && l != 0.0f && ((l > 0.0f) == (k.det > 0.0f));
    uint32_t ws = 0u, s0 = 0u, s1 = 0u, s2 = 0u, s3 = 0u, cmin = 255u;
    if (front) {
        const float sx = div_spec(a, l), sy = div_spec(b, l);
        const float qx = ((sx + 1.0f) * 0.5f) * k.W - 0.5f;
        const float qy = ((sy + 1.0f) * 0.5f) * k.H - 0.5f;
        o.mvx = qx - (float)px; o.mvy = qy - (float)py;      // 3. motion, inside the frame or not
        if (hs != nullptr && rp_finite(qx) && rp_finite(qy)) { // 4. taps and weights
            const float x0f = floorf(qx), y0f = floorf(qy);
            const int wx = (int)floorf((qx - x0f) * 256.0f + 0.5f), wy = (int)floorf((qy - y0f) * 256.0f + 0.5f);
            // (clamped before the conversion: beyond [-1, W - 1] no tap lies inside the frame, however far beyond)
            const int x0 = (int)fminf(fmaxf(x0f, -2.0f), k.W), y0 = (int)fminf(fmaxf(y0f, -2.0f), k.H);
            const f3 dc = mk3(P.x - k.cur_pos.x, P.y - k.cur_pos.y, P.z - k.cur_pos.z);
            const float tol = k.tol_abs + k.tol_rel * len3(dc);
            const float tol2 = tol * tol;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
            for (int t = 0; t < 4; t++) {
                const int tx = x0 + (t & 1), ty = y0 + (t >> 1);
                const uint32_t w = (uint32_t)((t & 1) ? wx : 256 - wx) * (uint32_t)((t >> 1) ? wy : 256 - wy);
                if (w == 0u || tx < 0 || tx >= k.Wi || ty < 0 || ty >= k.Hi) continue;
                const size_t idx = (size_t)ty * (size_t)k.Wi + (size_t)tx;
#if defined(__HIP_DEVICE_COMPILE__)
                // position, normal and count in ONE 16-byte load (as a struct the compiler fetches w first and xyz behind the
                // normal test: two dependent trips to L2 per tap)
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

} // namespace vrt
