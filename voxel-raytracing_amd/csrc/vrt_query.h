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
// for the budgets that loop accepts (maxSteps <= 1024; vrt_march_fast.h, df_fast_loop).
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

// Directions at the bottom of the float range.  A component is "small" when it is +-0 or subnormal (|d| < 2^-126).
//  * All three small but not all zero: outside the contract (include/vrt.h: GLSL may flush subnormals to zero, and where it does
//    not, the three sideDist are infinite or overflow within a few steps and the reference's loop steps every axis on the tie).
//    query_ray takes the flushing reading, on the device and on the host: every component becomes a zero of its own sign, a direction whose march
//    stands still.  Without it VRT_TRAVERSAL_DF would recover a position from an overflowed sideDist (inf * g, g subnormal, converts
//    to INT_MAX) and index the fields with it.
//  * One or two subnormal beside an ordinary one: in the contract.  query_subnormal_component says so; k_query sends the wave
//    through VRT_TRAVERSAL_DF instead of the look-up loop.
VRT_HD bool query_small(float d) { return (f2u(d) & 0x7F800000u) == 0u; }
VRT_HD void query_flush_direction(f3& dir)
{
    if (query_small(dir.x) && query_small(dir.y) && query_small(dir.z))        // (each component keeps its sign: -0.0 stays -0.0)
        dir = mk3(u2f(f2u(dir.x) & 0x80000000u), u2f(f2u(dir.y) & 0x80000000u), u2f(f2u(dir.z) & 0x80000000u));
}
VRT_HD bool query_subnormal_component(f3 dir)
{
    return (query_small(dir.x) && dir.x != 0.0f) || (query_small(dir.y) && dir.y != 0.0f) || (query_small(dir.z) && dir.z != 0.0f);
}

// Origins far from the volume.  The budget-free marches (df_prim_loop, brick_march_thresh) are entered by a wave none of whose rays
// can reach max_steps, judged by tspan * (|dx| + |dy| + |dz|) * 1.001 + 8 (trace_df_fast).  tspan = tmax - t0 is a difference of two
// t = (plane - origin) / d, each wrong by up to two ulps of its own size: in steps, up to about 2^-22 * 3 * |origin| along the
// longest axis.  For |origin| <= 2^20 that is below one step, well inside the margin of 8; beyond, it can exceed it, and an
// under-bounded ray would march past its budget.  k_query therefore clears df_thresh for a wave that holds such an origin.
VRT_HD bool query_far_origin(f3 start)
{
    const float lim = 1048576.0f;
    return !(fabsf(start.x) <= lim && fabsf(start.y) <= lim && fabsf(start.z) <= lim);
}

// One ray of a query.  TRAV: what VRT_TRAVERSAL_AUTO resolves to for the scene (VRT_TRAVERSAL_DF_FAST, _DF or _BRICK);
// ANYHIT: traceRayHit (frag:198-202), only h.material is defined.  Wave-cooperative on the device like the march itself:
// every lane of a wave calls it, a lane without a ray with one that ends before it starts (query_no_ray).
template <int TRAV, bool ANYHIT>
VRT_HD void query_ray(const VolumeView& v, f3 start, f3 dir, uint32_t maxSteps, QueryHit& h)
{
    RayInt r;
    query_flush_direction(dir);
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
