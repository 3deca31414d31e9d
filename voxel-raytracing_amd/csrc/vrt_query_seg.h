// vrt_query_seg.h -- ray segments (vrt_trace_segments, vrt_occluded_segments): a ray query with a distance limit per ray.  What
// vrt_query.h defines stays as it is; this header adds the hit's parameter along the ray, the rule that drops a hit beyond the
// limit, and a bound on the iterations a hit within the limit can need.  Compiled for the device by vrt_query_seg.hip and for the
// host by tests/native/segment_host.cpp (against the oracle's vo_trace_ray and tests/segment_reference.py, without a GPU).
//
//   t_hit = t_adv + d    one fp32 addition.  d is the length query_hit_record multiplies dir by (RayHit.pos = p + d * dir, frag:187-189);
//                        t_adv is what boxIntersection moved the origin by to get p: tmin + 0.1 where its test passes (frag:120-123),
//                        else 0.  Both are in units of dir, like the +0.1: a direction twice as long halves every t.
//   kept  iff  t_hit <= t_max, an fp32 compare: a NaN t_max keeps nothing, +inf everything, and 0 (either sign) a ray that starts
//                        inside a solid voxel (t_adv = 0, d = 0).  A dropped hit is a miss: 0 in every plane, t included.
// Everything else is vrt_trace_rays' contract: the same open set (include/vrt.h, (1) - (4)), the same reading of a direction whose
// components are all zero or subnormal.
#pragma once

#include "vrt_query.h"

namespace vrt {

// boxIntersection's tmin and tmax (frag:111-119) by dda_entry's own expressions in its own order (vrt_dda.h: DdaState keeps neither)
VRT_HD void query_box_t(const VolumeView& v, f3 start, f3 dir, float& tmin, float& tmax)
{
    float ivx = 1.0f / dir.x, ivy = 1.0f / dir.y, ivz = 1.0f / dir.z;
    float t1x = (-start.x) * ivx, t2x = ((float)v.W - start.x) * ivx;
    float t1y = (-start.y) * ivy, t2y = ((float)v.H - start.y) * ivy;
    float t1z = (-start.z) * ivz, t2z = ((float)v.D - start.z) * ivz;
    float tnx = fminf(t1x, t2x), tny = fminf(t1y, t2y), tnz = fminf(t1z, t2z);
    float txx = fmaxf(t1x, t2x), txy = fmaxf(t1y, t2y), txz = fmaxf(t1z, t2z);
    tmin = fmaxf(tnx, fmaxf(tny, tnz));
    tmax = fminf(txx, fminf(txy, txz));
}

// The parameter of r's hit along the ray (start, dir) as given to the query; 0 for a miss.  r: the finished march of that ray.
VRT_HD float query_hit_t(const VolumeView& v, f3 start, f3 dir, const RayInt& r)
{
    if (r.material == 0) return 0.0f;
    query_flush_direction(dir);                                // (the direction query_ray marched)
    float tmin, tmax;
    query_box_t(v, start, dir, tmin, tmax);
    const float t_adv = (tmin >= 0.0f && tmax >= tmin) ? tmin + 0.1f : 0.0f;
    f3 m = mk3((r.mask & 1u) ? (r.side.x - r.delta.x) : 0.0f,
               (r.mask & 2u) ? (r.side.y - r.delta.y) : 0.0f,
               (r.mask & 4u) ? (r.side.z - r.delta.z) : 0.0f);
    const float d = len3(m);                                   // query_hit_record's d
    return t_adv + d;
}

VRT_HD bool query_segment_keeps(uint32_t material, float t_hit, float t_max) { return material != 0u && t_hit <= t_max; }

// At least the number of loop iterations the reference needs to report any hit of the ray with t_hit <= t_max -- a hit in
// iteration k (counted from 0) needs a budget of k + 1 --, or +inf where this function does not bound them.
//
// An iteration that does not hit steps at least one axis, and an axis steps once per integer plane the ray crosses, so a hit in
// iteration k lies at least k plane crossings behind boxIntersection's point p.  Between p (parameter t_adv) and the hit (t_hit)
// axis a crosses at most (t_hit - t_adv) * |dir.a| + 1 planes, in all no more than  (t_hit - t_adv) * (|dx| + |dy| + |dz|) + 3.
// t_hit <= t_max, and t_adv >= t0 = max(tmin, 0) -- it is tmin + 0.1 where the box test passes and 0 where tmin < 0; a ray
// with tmin >= 0 that fails the test never enters the volume and has no hit to bound --, so the span is at most t_max - t0; and
// a hit lies inside the box, so it is at most tspan = tmax - t0 as well (vrt_march_fast.h: the bound that admits a wave to
// the budget-free loop is this one at t_max = +inf).  What fp32 adds, and the margin (x 1.001, + 8 instead of + 3) covers:
//  * d is made of a sideDist that k additions of deltaDist built: wrong by at most k 2^-24 of itself, below 0.00074 for the
//    k <= 3 * 4096 a volume of the documented size allows: the factor 1.001;
//  * tmin and tmax are each wrong by up to two ulps of their own size, t_hit = t_adv + d and t_max - t0 by half an ulp of theirs:
//    in steps together below 2^-21 * 3 * |origin| along the longest axis, under two steps for |origin| <= 2^20 (query_far_origin);
//  * the rounding of the sum of the three |dir| and of the two products: relative 2^-22, in the factor as well.
// That leaves three of the eight steps unused.  Beyond 2^20 the second item grows past any fixed margin, and a NaN t_max keeps no
// hit at all: both give +inf, as does a product that is not finite (a span of +inf times a zero sum: the direction (0, 0, 0)).
VRT_HD float query_segment_bound(const VolumeView& v, f3 start, f3 dir, float t_max)
{
    const float kInf = u2f(0x7F800000u);
    if (query_far_origin(start) || t_max != t_max) return kInf;
    query_flush_direction(dir);
    float tmin, tmax;
    query_box_t(v, start, dir, tmin, tmax);
    const float t0 = fmaxf(tmin, 0.0f);
    const float tspan = tmax >= t0 ? tmax - t0 : 0.0f;         // dda_entry's
    const float span = fminf(fmaxf(t_max - t0, 0.0f), tspan);
    const float bound = span * ((fabsf(dir.x) + fabsf(dir.y)) + fabsf(dir.z)) * 1.001f + 8.0f;
    return bound < kInf ? bound : kInf;                        // (NaN -> +inf)
}

// One ray of a segment query: query_ray's closest-hit march with the budget the caller gives (max_steps, or the wave's segment
// budget), then the segment rule.  ANYHIT: only h.material is defined (the id of a kept hit, else 0) -- the march is the
// closest-hit one all the same, because only that march holds the final sideDist t_hit is made from.
template <int TRAV, bool ANYHIT>
VRT_HD void query_segment_ray(const VolumeView& v, f3 start, f3 dir, float t_max, uint32_t maxSteps, QueryHit& h, float& t)
{
    RayInt r;
    f3 fdir = dir;
    query_flush_direction(fdir);
    trace_int<TRAV, const uint64_t*, false, false>(v, v.occ2, v.occ3, start, fdir, maxSteps, r);
    t = query_hit_t(v, start, dir, r);
    const bool keep = query_segment_keeps(r.material, t, t_max);
    if (!keep) t = 0.0f;
    if (ANYHIT) { h.material = keep ? r.material : 0u; return; }
    int mx = r.mx, my = r.my, mz = r.mz;
    if (TRAV == VRT_TRAVERSAL_DF_FAST) query_recover_voxel(r, fdir, mx, my, mz);
    if (!keep) r.material = 0u;                                // query_hit_record writes a miss as zeros
    query_hit_record(r, fdir, mx, my, mz, h);
}

} // namespace vrt
