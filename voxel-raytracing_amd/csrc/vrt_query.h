// vrt_query.h -- ray queries (vrt_trace_rays, vrt_occluded_rays, vrt_pick_pixels): what a query returns for one ray, made
// from the march's finished RayInt.  Compiled for the device by vrt_query.hip and for the host by
// tests/native/query_host.cpp (against the oracle's vo_trace_ray, without a GPU).
//
// The record is traceRay's (voxel_volume.frag:176-196) with the normal before its normalisation:
//   material  voxel id at the hit, 0 = miss (a ray that leaves the volume, or exhausts maxSteps)
//   pos       RayHit.pos = boxIntersection's point + length(mask * (sideDist - deltaDist)) * dir -- the expression, in the
//             order, of vrt_shade.h's trace_ray, so a primary ray's pos is the position plane's, bit for bit
//   voxel     mapPos at the hit
//   normal    -mask * rayStep, every component in {-1, 0, 1}
// and zeros in every field of a miss: the march ends a missing ray where nothing solid is left in its octant (open cells),
// so its last mapPos is not the reference loop's and is not reported.
#pragma once

#include "vrt_traverse.h"

namespace vrt {

struct QueryHit {
    uint32_t material;
    f3       pos;
    int32_t  vx, vy, vz;
    int32_t  nx, ny, nz;
};

// The hand-written look-up loop (trace_df_fast) keeps no mapPos: RayInt holds the FIRST one.  Where the ray stands is what
// the loop itself computes for every look-up: per axis n = rint(side * g + c) steps since the start of the ray, g = dir
// (1 / +-deltaDist to within an ulp; 0 for an axis the ray cannot step along) and c = -side0 * g, side0 the first sideDist
// (frag:142-144, recomputed here from the first mapPos as dda_rest does).  |error of n| <= (n^2 + 3n) 2^-24, below 1/16
// for the budgets that loop accepts (maxSteps <= 1024; vrt_traverse.h, df_fast_loop).
VRT_HD void query_recover_voxel(const RayInt& r, f3 dir, int& mx, int& my, int& mz)
{
    const float kInf = u2f(0x7F800000u);
    const float gx = (float)r.sx, gy = (float)r.sy, gz = (float)r.sz;
    const float s0x = ((gx * ((float)r.mx - r.pos.x) + gx * 0.5f) + 0.5f) * r.delta.x;
    const float s0y = ((gy * ((float)r.my - r.pos.y) + gy * 0.5f) + 0.5f) * r.delta.y;
    const float s0z = ((gz * ((float)r.mz - r.pos.z) + gz * 0.5f) + 0.5f) * r.delta.z;
    mx = r.mx + (r.delta.x < kInf ? steps_taken(r.side.x * dir.x + (-(s0x * dir.x))) : 0);
    my = r.my + (r.delta.y < kInf ? steps_taken(r.side.y * dir.y + (-(s0y * dir.y))) : 0);
    mz = r.mz + (r.delta.z < kInf ? steps_taken(r.side.z * dir.z + (-(s0z * dir.z))) : 0);
}

// (mx, my, mz): mapPos at the end of the march (r's own, or query_recover_voxel's)
VRT_HD void query_hit_record(const RayInt& r, f3 dir, int mx, int my, int mz, QueryHit& h)
{
    f3 pos = mk3(0.0f, 0.0f, 0.0f);
    int32_t vx = 0, vy = 0, vz = 0, nx = 0, ny = 0, nz = 0;
    if (r.material != 0) {
        f3 m = mk3((r.mask & 1u) ? (r.side.x - r.delta.x) : 0.0f,
                   (r.mask & 2u) ? (r.side.y - r.delta.y) : 0.0f,
                   (r.mask & 4u) ? (r.side.z - r.delta.z) : 0.0f);
        float d = len3(m);
        pos = mk3(r.pos.x + d * dir.x, r.pos.y + d * dir.y, r.pos.z + d * dir.z);
        vx = mx; vy = my; vz = mz;
        nx = (r.mask & 1u) ? -r.sx : 0; ny = (r.mask & 2u) ? -r.sy : 0; nz = (r.mask & 4u) ? -r.sz : 0;
    }
    h.material = r.material; h.pos = pos;
    h.vx = vx; h.vy = vy; h.vz = vz; h.nx = nx; h.ny = ny; h.nz = nz;
}

// One ray of a query.  TRAV: what VRT_TRAVERSAL_AUTO resolves to for the scene (VRT_TRAVERSAL_DF_FAST, _DF or _BRICK);
// ANYHIT: traceRayHit (frag:198-202), only h.material is defined.  Wave-cooperative on the device like the march itself:
// every lane of a wave calls it, a lane without a ray with one that ends before it starts (query_no_ray).
template <int TRAV, bool ANYHIT>
VRT_HD void query_ray(const VolumeView& v, f3 start, f3 dir, uint32_t maxSteps, QueryHit& h)
{
    RayInt r;
    trace_int<TRAV, const uint64_t*, false, ANYHIT>(v, v.occ2, v.occ3, start, dir, maxSteps, r);
    if (ANYHIT) { h.material = r.material; return; }
    int mx = r.mx, my = r.my, mz = r.mz;
    if (TRAV == VRT_TRAVERSAL_DF_FAST) query_recover_voxel(r, dir, mx, my, mz);
    query_hit_record(r, dir, mx, my, mz, h);
}

// A ray that is finished before it starts, for the lanes of a wave that have none (past the end of a batch, a pixel off the
// screen): the march's loops agree on run lengths over the whole wave, so such a lane may not leave the kernel -- it starts
// outside the volume pointing away from it, boxIntersection misses, and iteration 0 finds its mapPos out of bounds.
VRT_HD void query_no_ray(f3& start, f3& dir)
{
    start = mk3(-1.0f, -1.0f, -1.0f); dir = mk3(-1.0f, -1.0f, -1.0f);
}

} // namespace vrt
