// vrt_render_rays.h -- vrt_render_rays: what the G-buffer of a caller-supplied primary ray holds, made from the march's finished
// RayInt, and the record its hit hands to the shading kernel.  Compiled for the device by vrt_render_rays.hip and for the host by
// tests/native/render_rays_host.cpp (against the oracle's main(), without a GPU).
//
// The primary record is vrt_trace_rays' (vrt_query.h: the same flushing of an all-small direction, the same march, the same
// position expression, query_recover_voxel on the hand-written loop); the planes are K1's (vrt_device.hip, k_primary) with the
// caller's origin where K1 has the camera position; the packed word is k_primary MODE 0's, which k_shade unpacks.
#pragma once

#include "vrt_query.h"

namespace vrt {

// K2's record word: material | mask << 8 | (rayStep + 1) codes, two bits per axis from bit 11
VRT_HD uint32_t rays_pack(uint32_t material, uint32_t mask, int sx, int sy, int sz)
{
    return material | (mask << 8) | ((uint32_t)(sx + 1) << 11) | ((uint32_t)(sy + 1) << 13) | ((uint32_t)(sz + 1) << 15);
}
VRT_HD void rays_unpack(uint32_t w, uint32_t& material, uint32_t& mask, int& sx, int& sy, int& sz)
{
    material = w & 0xFFu;
    mask = (w >> 8) & 7u;
    sx = (int)((w >> 11) & 3u) - 1; sy = (int)((w >> 13) & 3u) - 1; sz = (int)((w >> 15) & 3u) - 1;
}

// normalize(-mask * rayStep) (frag:190) as vrt_shade.h's hit_normal computes it -- the same lines, here for host and device: the
// shading header is device only, and K1 / K2 must not change with this file
VRT_HD f3 rays_hit_normal(uint32_t mask, int sx, int sy, int sz)
{
    const uint32_t k = (uint32_t)__builtin_popcount(mask & 7u);
    const float c = k == 1u ? 1.0f : (k == 2u ? u2f(0x3f3504f3u) : u2f(0x3f13cd3au));
    const bool general = ((mask & 1u) && sx == 0) || ((mask & 2u) && sy == 0) || ((mask & 4u) && sz == 0);
    f3 n = mk3((mask & 1u) ? (float)(-sx) : 0.0f, (mask & 2u) ? (float)(-sy) : 0.0f, (mask & 4u) ? (float)(-sz) : 0.0f);
    if (general) return normalize3(n);
    return mk3(n.x * c, n.y * c, n.z * c);
}

// One pixel of the G-buffer, every plane but the colour (a miss: zeros), and the hit's record word
struct RaysPixel {
    float    depth;                 // len3(pos - origin)
    f3       pos;                   // position = (pos, 0)
    uint32_t normal8;               // snorm8 codes of the normal: x | y << 8 | z << 16
    uint8_t  mask8, hit_id, hit_mask;
    int16_t  vx, vy, vz;            // hit_voxel
    uint32_t packed;                // rays_pack of the hit (0 on a miss)
};

// r: the finished march of the ray (start, dir); h: its query record (query_hit_record: pos and the hit cell)
VRT_HD void rays_pixel(const RayInt& r, const QueryHit& h, f3 start, RaysPixel& g)
{
    const bool hit = r.material != 0u;
    g.depth = 0.0f;
    if (hit) g.depth = len3(mk3(h.pos.x - start.x, h.pos.y - start.y, h.pos.z - start.z));
    g.pos = h.pos;
    g.normal8 = 0u;
    if (hit) {
        const f3 n = rays_hit_normal(r.mask, r.sx, r.sy, r.sz);
        g.normal8 = (uint32_t)(uint8_t)snorm8(n.x) | ((uint32_t)(uint8_t)snorm8(n.y) << 8) | ((uint32_t)(uint8_t)snorm8(n.z) << 16);
    }
    g.mask8 = hit ? (uint8_t)230 : (uint8_t)0;                 // unorm8(0.9f) = 230
    g.hit_id = (uint8_t)r.material;
    g.hit_mask = hit ? (uint8_t)r.mask : (uint8_t)0;
    g.vx = (int16_t)h.vx; g.vy = (int16_t)h.vy; g.vz = (int16_t)h.vz;
    g.packed = hit ? rays_pack(r.material, r.mask, r.sx, r.sy, r.sz) : 0u;
}

// The primary ray of a pixel: query_ray's closest-hit march (vrt_query.h) with the RayInt kept.  Wave-cooperative on the device
// like the march itself: every lane of the wave calls it, a lane without a ray with query_no_ray's.
template <int TRAV>
VRT_HD void rays_primary(const VolumeView& v, f3 start, f3 dir, uint32_t maxSteps, RayInt& r, QueryHit& h)
{
    query_flush_direction(dir);
    trace_int<TRAV, const uint64_t*, false, false>(v, v.occ2, v.occ3, start, dir, maxSteps, r);
    int mx = r.mx, my = r.my, mz = r.mz;
    if (TRAV == VRT_TRAVERSAL_DF_FAST) query_recover_voxel(r, dir, mx, my, mz);
    query_hit_record(r, dir, mx, my, mz, h);
}

} // namespace vrt
