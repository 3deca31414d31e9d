// vrt_render_rays.hip -- vrt_render_rays: the G-buffer of a frame whose primary rays the caller supplies, in the split form
// the render stage already has (k_primary MODE 0 -> records -> k_shade), fed from a ray buffer.  An object of its own: the
// render stage's kernels (vrt_device.hip) and the ray queries' (vrt_query.hip) do not see this file.
//
//   k_rays_primary<TRAV>   k_query's launch shape and routing (one ray per lane, one wave per workgroup, no lane leaves before
//                          the march): marches ray i, writes pixel i of every plane but a hit's colour, the sky colour of a
//                          miss, and for a hit K2's record and an entry of the compacted hit list
//   k_shade_rays<TRAV>     k_shade's body (one lane per hit of the list, 256 lanes and 4 * VRT_AO_SLOT bytes of LDS per
//                          workgroup) with h.dir read from the caller's dirs plane instead of primary_dir
//
// What each of them owes the code it calls (vrt_shade.h's launch contract; k_query's assumptions): DESIGN.md 4, "render rays".
#include "vrt_shade.h"
#include "vrt_frame_slot.h"     // OccT, gptr (nothing here reads the kernel-argument segment: no kernarg_words, no SlotOf)
#include "vrt_render_rays.h"

namespace vrt {

// three dwords per ray through the wave's LDS, as k_query fetches them (vrt_query.hip, wave_fetch: whole-dword, lane-contiguous
// loads; a lane takes its three at stride 3).  The same lines: k_query must not change with this file.
__device__ __forceinline__ void rays_fetch3(const uint32_t* __restrict__ src, uint32_t base, uint32_t n, uint32_t* lds, uint32_t lane, uint32_t (&out)[3])
{
    const uint32_t first = base * 3u, total = n * 3u;          // (n < 2^28: no overflow)
#pragma unroll
    for (int q = 0; q < 3; q++) {
        const uint32_t idx = first + (uint32_t)q * 64u + lane;
        lds[q * 64 + lane] = idx < total ? src[idx] : 0u;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 3; k++) out[k] = lds[lane * 3 + k];
    __syncthreads();
}

template <int TRAV>
__global__ __launch_bounds__(64) void k_rays_primary(const RaysParams P)
{
    __shared__ uint32_t lds[192];
    const uint32_t lane = threadIdx.x, base = blockIdx.x * 64u, n = P.n;
    const uint32_t i = base + lane;
    const bool live = i < n;
    uint32_t o[3], d[3];
    rays_fetch3(reinterpret_cast<const uint32_t*>(P.origins), base, n, lds, lane, o);
    rays_fetch3(reinterpret_cast<const uint32_t*>(P.dirs), base, n, lds, lane, d);
    f3 start = mk3(__uint_as_float(o[0]), __uint_as_float(o[1]), __uint_as_float(o[2]));
    f3 dir = mk3(__uint_as_float(d[0]), __uint_as_float(d[1]), __uint_as_float(d[2]));
    // no lane leaves before the march: its loops vote over the whole wave (vrt_query.h, query_no_ray)
    if (!live) query_no_ray(start, dir);
    // k_query's routing, wave-uniform: a subnormal direction component sends the wave through VRT_TRAVERSAL_DF, a far origin
    // keeps it out of the budget-free march (vrt_query.h)
    VolumeView vol = P.sc.vol;
    if (__any(query_far_origin(start)) != 0) vol.df_thresh = 0u;
    RayInt r; QueryHit h;
    if (TRAV == VRT_TRAVERSAL_DF_FAST && __any(query_subnormal_component(dir)) != 0)
        rays_primary<VRT_TRAVERSAL_DF>(vol, start, dir, P.max_steps, r, h);
    else
        rays_primary<TRAV>(vol, start, dir, P.max_steps, r, h);
    if (!live) return;                                         // (nothing below is wave-cooperative)

    RaysPixel g;
    rays_pixel(r, h, start, g);
    const vrt_frame& f = P.fr;
    // (32-bit byte offsets: the host admits frames below 2^28 pixels)
    if (f.depth) *gptr<float>(f.depth, i << 2) = g.depth;
    if (f.motion) *gptr<vrt_f2>(f.motion, i << 3) = (vrt_f2){0.0f, 0.0f};
    if (f.mask8) *gptr<uint8_t>(f.mask8, i) = g.mask8;
    if (f.position) *gptr<vrt_f4>(f.position, i << 4) = (vrt_f4){g.pos.x, g.pos.y, g.pos.z, 0.0f};
    if (f.normal8) *gptr<uint32_t>(f.normal8, i << 2) = g.normal8;
    if (f.hit_id) *gptr<uint8_t>(f.hit_id, i) = g.hit_id;
    if (f.hit_voxel) { f.hit_voxel[(size_t)i * 3 + 0] = g.vx; f.hit_voxel[(size_t)i * 3 + 1] = g.vy; f.hit_voxel[(size_t)i * 3 + 2] = g.vz; }
    if (f.hit_mask) *gptr<uint8_t>(f.hit_mask, i) = g.hit_mask;
    if (r.material != 0u) {
        // hit record for k_shade_rays and a slot in the compacted list of hits, as k_primary MODE 0 writes them
        P.records[i] = make_uint4(__float_as_uint(g.pos.x), __float_as_uint(g.pos.y), __float_as_uint(g.pos.z), g.packed);
        const uint32_t slot = atomicAdd(P.hit_count, 1u);
        P.hit_list[slot] = i;
    } else {
        // misses are final here (voxel_volume.frag:337-345): skyColor of the direction as given
        const f3 col = sky_color(P.sc, dir);
        if (f.color_f) { f.color_f[(size_t)i * 3 + 0] = col.x; f.color_f[(size_t)i * 3 + 1] = col.y; f.color_f[(size_t)i * 3 + 2] = col.z; }
        if (f.color8) *gptr<uint32_t>(f.color8, i << 2) = (uint32_t)unorm8(col.x) | ((uint32_t)unorm8(col.y) << 8) | ((uint32_t)unorm8(col.z) << 16);
    }
}

// k_shade (vrt_device.hip) over the hits of k_rays_primary.  P: a GeomParams built as for a split launch of one frame; slot 0
// holds the out planes and a push block of which the shading path reads `frame` alone.
template <int TRAV>
__global__ __launch_bounds__(256) void k_shade_rays(const GeomParams P, const float* __restrict__ dirs)
{
    extern __shared__ __attribute__((aligned(16))) uint64_t lds_occ[];
    uint32_t count = *P.hit_count;                        // written by k_rays_primary (previous kernel on the stream)
    if (blockIdx.x * 256u >= count) return;               // uniform per workgroup
    OccT<false> occ; occ.o2 = P.sc.vol.occ2; occ.o3 = P.sc.vol.occ3;
    uint32_t gid = blockIdx.x * 256u + threadIdx.x;
    if (gid >= count) return;
    size_t i = P.hit_list[gid];
    int W = P.W;
    int px = (int)(i % (size_t)W), py = (int)(i / (size_t)W);

    uint4 rec = P.records[i];
    RayHit h;
    h.material = rec.w & 0xFFu;
    h.dir = mk3(dirs[i * 3 + 0], dirs[i * 3 + 1], dirs[i * 3 + 2]);
    h.pos = mk3(__uint_as_float(rec.x), __uint_as_float(rec.y), __uint_as_float(rec.z));
    uint32_t mask = (rec.w >> 8) & 7u;
    int sx = (int)((rec.w >> 11) & 3u) - 1, sy = (int)((rec.w >> 13) & 3u) - 1, sz = (int)((rec.w >> 15) & 3u) - 1;
    PixCtx c; c.px = px; c.py = py; c.fetches = 0; c.rays = 0; c.pc = &P.slot[0].pc;
    c.ldsw = (uint32_t)(uintptr_t)(lds_u64_ptr)lds_occ + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) * (uint32_t)VRT_AO_SLOT;
    h.normal = hit_normal(mask, sx, sy, sz);
    {
        const bool general = (mask & 7u) == 0u || ((mask & 1u) && sx == 0) || ((mask & 2u) && sy == 0) || ((mask & 4u) && sz == 0);
        h.ncode = general ? 0xFFFFFFFFu : ((mask & 7u) | ((uint32_t)(sx < 0) << 3) | ((uint32_t)(sy < 0) << 4) | ((uint32_t)(sz < 0) << 5));
    }
    f3 col = color_main_ray<TRAV>(P, occ, c, h);
    const vrt_frame& f = P.slot[0].fr;
    if (f.color_f) { f.color_f[i * 3 + 0] = col.x; f.color_f[i * 3 + 1] = col.y; f.color_f[i * 3 + 2] = col.z; }
    if (f.color8) {
        uchar4 c8; c8.x = unorm8(col.x); c8.y = unorm8(col.y); c8.z = unorm8(col.z); c8.w = 0;
        reinterpret_cast<uchar4*>(f.color8)[i] = c8;
    }
}

hipError_t launch_rays_primary(const RaysParams& rp, int traversal, hipStream_t s)
{
    if (rp.n == 0u) return hipSuccess;
    const dim3 grid((rp.n + 63u) / 64u), block(64);
    if (traversal == VRT_TRAVERSAL_DF_FAST)    hipLaunchKernelGGL((k_rays_primary<VRT_TRAVERSAL_DF_FAST>), grid, block, 0, s, rp);
    else if (traversal == VRT_TRAVERSAL_BRICK) hipLaunchKernelGGL((k_rays_primary<VRT_TRAVERSAL_BRICK>), grid, block, 0, s, rp);
    else if (traversal == VRT_TRAVERSAL_DF)    hipLaunchKernelGGL((k_rays_primary<VRT_TRAVERSAL_DF>), grid, block, 0, s, rp);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_rays_shade(const GeomParams& p, const float* dirs, uint32_t n, int traversal, hipStream_t s)
{
    if (n == 0u) return hipSuccess;
    // one lane per hit of the compacted list; sized for the worst case (every ray hit), surplus workgroups leave at once.
    // VRT_AO_SLOT bytes of LDS per wave (vrt_shade.h, clause 1), whatever the traversal
    const dim3 grid((n + 255u) / 256u), block(256);
    const size_t lds = 4u * (size_t)VRT_AO_SLOT;
    if (traversal == VRT_TRAVERSAL_DF_FAST)    hipLaunchKernelGGL((k_shade_rays<VRT_TRAVERSAL_DF_FAST>), grid, block, lds, s, p, dirs);
    else if (traversal == VRT_TRAVERSAL_BRICK) hipLaunchKernelGGL((k_shade_rays<VRT_TRAVERSAL_BRICK>), grid, block, lds, s, p, dirs);
    else if (traversal == VRT_TRAVERSAL_DF)    hipLaunchKernelGGL((k_shade_rays<VRT_TRAVERSAL_DF>), grid, block, lds, s, p, dirs);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

} // namespace vrt
