// vrt_query.hip -- ray queries: the marches behind vrt_traverse.h (vrt_march_*.h) fed from a ray buffer (vrt_trace_rays, vrt_occluded_rays) or
// from pixel coordinates (vrt_pick_pixels) instead of a frame's pixels.  An object of its own: the render stage's kernels
// (vrt_device.hip) do not see this file.
//
//   k_query<TRAV, ANYHIT, PICK>   one ray per lane, one wave per workgroup (a wave slot is free again the moment its 64 rays
//                                 are done, as in K1), rays in the order given.
//
// Memory: a lane's ray is 2 x 12 bytes and its record up to 1 + 12 + 12 + 3 bytes, in planes of three values per ray.  A
// lane reading or writing its own three values would touch addresses 12 bytes apart: three instructions that each span 768
// bytes.  So every plane goes through the wave's LDS instead: the wave's 192 dwords (48 for the normals) are moved with
// whole-dword, lane-contiguous instructions (lane l: dword 64q + l, q = 0..2 -- full 256-byte lines) and a lane takes its
// three from LDS at stride 3, which is free of bank conflicts (3 is odd).  The one-byte planes are lane-contiguous as they are.
#include "vrt_device_common.h"
#include "vrt_query.h"
#include "vrt_query_io.h"

namespace vrt {

template <int TRAV, bool ANYHIT, bool PICK>
__global__ __launch_bounds__(64) void k_query(const QueryParams P)
{
    __shared__ uint32_t lds[192];
    const uint32_t lane = threadIdx.x, base = blockIdx.x * 64u, n = P.n;
    const uint32_t i = base + lane;
    bool live = i < n;                                         // this lane has a ray of the batch ...
    bool on = live;                                            // ... that is traced (PICK: its pixel is on the screen)
    f3 start, dir;
    if (PICK) {
        uint32_t xy[2];
        wave_fetch<2>(reinterpret_cast<const uint32_t*>(P.xy), base, n, lds, lane, xy);
        const int px = (int)xy[0], py = (int)xy[1];
        on = live && px >= 0 && py >= 0 && px < P.W && py < P.H;
        // main()'s ray as K1 builds it (vrt_device_common.h); a lane without a pixel computes pixel (0, 0)'s and does not use it
        const f3 v = primary_v(P.rg, P.cam_right[0], P.cam_right[1], P.cam_right[2], P.rcp_w, P.rcp_h, P.fast_screen_div, on ? px : 0, on ? py : 0);
        dir = primary_normalize(v);
        start = mk3(P.cam_pos[0], P.cam_pos[1], P.cam_pos[2]);
    } else {
        uint32_t o[3], d[3];
        wave_fetch<3>(reinterpret_cast<const uint32_t*>(P.origins), base, n, lds, lane, o);
        wave_fetch<3>(reinterpret_cast<const uint32_t*>(P.dirs), base, n, lds, lane, d);
        start = mk3(__uint_as_float(o[0]), __uint_as_float(o[1]), __uint_as_float(o[2]));
        dir = mk3(__uint_as_float(d[0]), __uint_as_float(d[1]), __uint_as_float(d[2]));
    }
    // no lane leaves before the march: its loops vote over the whole wave (vrt_query.h, query_no_ray)
    if (!on) query_no_ray(start, dir);
    QueryHit h;
    // The look-up loop recovers positions as side * g + c with g = dir: for a subnormal component that is a product of a huge
    // and a subnormal factor in an instruction (v_mul_legacy_f32) whose treatment of subnormals the loop's bounds do not cover,
    // so a wave that holds such a ray takes VRT_TRAVERSAL_DF, which only ever multiplies the sideDist travelled in a run -- exactly
    // 0 for an axis that did not step (vrt_query.h, query_subnormal_component).  Wave-uniform: the march's loops vote.
    // ... and a wave that holds an origin too far away for the bound that admits a wave to the budget-free march does not take it
    // (vrt_query.h, query_far_origin)
    VolumeView vol = P.vol;
    if (__any(query_far_origin(start)) != 0) vol.df_thresh = 0u;
    if (TRAV == VRT_TRAVERSAL_DF_FAST && __any(query_subnormal_component(dir)) != 0)
        query_ray<VRT_TRAVERSAL_DF, ANYHIT>(vol, start, dir, P.max_steps, h);
    else
        query_ray<TRAV, ANYHIT>(vol, start, dir, P.max_steps, h);
    if (!on) { h.material = 0u; h.pos = mk3(0.0f, 0.0f, 0.0f); h.vx = h.vy = h.vz = 0; h.nx = h.ny = h.nz = 0; }

    if (ANYHIT) {
        if (live) P.material[i] = h.material != 0u ? (uint8_t)1 : (uint8_t)0;
        return;
    }
    if (P.material && live) P.material[i] = (uint8_t)h.material;
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
static void launch_query_t(const QueryParams& p, int anyhit, int pick, dim3 grid, hipStream_t s)
{
    if (pick)        hipLaunchKernelGGL((k_query<TRAV, false, true>), grid, dim3(64), 0, s, p);
    else if (anyhit) hipLaunchKernelGGL((k_query<TRAV, true, false>), grid, dim3(64), 0, s, p);
    else             hipLaunchKernelGGL((k_query<TRAV, false, false>), grid, dim3(64), 0, s, p);
}

hipError_t launch_query(const QueryParams& p, int traversal, int anyhit, int pick, hipStream_t s)
{
    if (p.n == 0u) return hipSuccess;
    const dim3 grid((p.n + 63u) / 64u);
    if (traversal == VRT_TRAVERSAL_DF_FAST)    launch_query_t<VRT_TRAVERSAL_DF_FAST>(p, anyhit, pick, grid, s);
    else if (traversal == VRT_TRAVERSAL_BRICK) launch_query_t<VRT_TRAVERSAL_BRICK>(p, anyhit, pick, grid, s);
    else if (traversal == VRT_TRAVERSAL_DF)    launch_query_t<VRT_TRAVERSAL_DF>(p, anyhit, pick, grid, s);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

} // namespace vrt
