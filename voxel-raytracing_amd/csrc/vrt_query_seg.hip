// vrt_query_seg.hip -- ray segments (vrt_trace_segments, vrt_occluded_segments): k_query's ray buffers with a distance limit per ray
// (vrt_query_seg.h).  An object of its own: neither the render stage's kernels nor k_query see this file.
//
//   k_query_seg<TRAV, ANYHIT>   one ray per lane, one wave per workgroup, the 3-dword planes through the wave's LDS (vrt_query_io.h);
//                               t_max is read and t written one dword per ray, lane-contiguous as they are.
//
// Both forms run the closest-hit march: t_hit is made from the final sideDist, which only that march holds.  What a segment saves is
// budget: the march takes its budget as a wave-uniform value, so a wave whose 64 segments are all short is marched with the few
// iterations they can need (query_segment_bound) instead of max_steps.  That never changes a result -- a hit within t_max is found
// inside the bound, a hit beyond it is dropped either way, a miss is a miss -- and it sits behind the context option "segment_budget".
#include "vrt_device_common.h"
#include "vrt_query_seg.h"
#include "vrt_query_io.h"

namespace vrt {

// max over the wave's 64 lanes of a non-negative float that is not NaN (the order of such floats is the order of their bit
// patterns), in a scalar register
__device__ __forceinline__ float wave_max_nonneg(float x)
{
    uint32_t b = __float_as_uint(x);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)b, o, 64);
        b = other > b ? other : b;
    }
    return __uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane((int)b));
}

template <int TRAV, bool ANYHIT>
__global__ __launch_bounds__(64) void k_query_seg(const QuerySegParams P)
{
    __shared__ uint32_t lds[192];
    const uint32_t lane = threadIdx.x, base = blockIdx.x * 64u, n = P.n;
    const uint32_t i = base + lane;
    const bool live = i < n;
    f3 start, dir;
    uint32_t o[3], d[3];
    wave_fetch<3>(reinterpret_cast<const uint32_t*>(P.origins), base, n, lds, lane, o);
    wave_fetch<3>(reinterpret_cast<const uint32_t*>(P.dirs), base, n, lds, lane, d);
    start = mk3(__uint_as_float(o[0]), __uint_as_float(o[1]), __uint_as_float(o[2]));
    dir = mk3(__uint_as_float(d[0]), __uint_as_float(d[1]), __uint_as_float(d[2]));
    const float t_max = live ? P.t_max[i] : 0.0f;
    // no lane leaves before the march: its loops vote over the whole wave (vrt_query.h, query_no_ray)
    if (!live) query_no_ray(start, dir);
    // k_query's rules for a wave that holds a far origin or a subnormal direction component
    VolumeView vol = P.vol;
    if (__any(query_far_origin(start)) != 0) vol.df_thresh = 0u;
    // The wave's budget: what its longest segment can need, where every lane's is bounded (+inf: a far origin, a NaN t_max, a
    // span the bound cannot multiply); a lane without a ray asks for nothing.  Wave-uniform, in a scalar register, like max_steps.
    // A wave whose limits are all +inf has nothing to save: it skips the bound and its reduction (one ballot instead).
    uint32_t budget = P.max_steps;
    if (P.wave_budget != 0u && __any(live && !(t_max == __uint_as_float(0x7F800000u))) != 0) {
        const float need = wave_max_nonneg(live ? query_segment_bound(vol, start, dir, t_max) : 0.0f);
        if (need < (float)budget) budget = (uint32_t)ceilf(need);          // (need >= 8: the budget stays >= 1)
    }
    QueryHit h;
    float t;
    if (TRAV == VRT_TRAVERSAL_DF_FAST && __any(query_subnormal_component(dir)) != 0)
        query_segment_ray<VRT_TRAVERSAL_DF, ANYHIT>(vol, start, dir, t_max, budget, h, t);
    else
        query_segment_ray<TRAV, ANYHIT>(vol, start, dir, t_max, budget, h, t);

    if (ANYHIT) {
        if (live) P.material[i] = h.material != 0u ? (uint8_t)1 : (uint8_t)0;
        return;
    }
    if (!live) { h.material = 0u; h.pos = mk3(0.0f, 0.0f, 0.0f); h.vx = h.vy = h.vz = 0; h.nx = h.ny = h.nz = 0; t = 0.0f; }
    if (P.material && live) P.material[i] = (uint8_t)h.material;
    if (P.t && live) P.t[i] = t;
    if (P.pos) {
        const uint32_t v[3] = {__float_as_uint(h.pos.x), __float_as_uint(h.pos.y), __float_as_uint(h.pos.z)};
        wave_store<3>(reinterpret_cast<uint32_t*>(P.pos), base, n, lds, lane, v);
    }
    if (P.voxel) {
        const uint32_t v[3] = {(uint32_t)h.vx, (uint32_t)h.vy, (uint32_t)h.vz};
        wave_store<3>(reinterpret_cast<uint32_t*>(P.voxel), base, n, lds, lane, v);
    }
    if (P.normal) wave_store_normals(P.normal, base, n, lds, lane, live, h.nx, h.ny, h.nz);
}

template <int TRAV>
static void launch_query_seg_t(const QuerySegParams& p, int anyhit, dim3 grid, hipStream_t s)
{
    if (anyhit) hipLaunchKernelGGL((k_query_seg<TRAV, true>), grid, dim3(64), 0, s, p);
    else        hipLaunchKernelGGL((k_query_seg<TRAV, false>), grid, dim3(64), 0, s, p);
}

hipError_t launch_query_seg(const QuerySegParams& p, int traversal, int anyhit, hipStream_t s)
{
    if (p.n == 0u) return hipSuccess;
    const dim3 grid((p.n + 63u) / 64u);
    if (traversal == VRT_TRAVERSAL_DF_FAST)    launch_query_seg_t<VRT_TRAVERSAL_DF_FAST>(p, anyhit, grid, s);
    else if (traversal == VRT_TRAVERSAL_BRICK) launch_query_seg_t<VRT_TRAVERSAL_BRICK>(p, anyhit, grid, s);
    else if (traversal == VRT_TRAVERSAL_DF)    launch_query_seg_t<VRT_TRAVERSAL_DF>(p, anyhit, grid, s);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

} // namespace vrt
