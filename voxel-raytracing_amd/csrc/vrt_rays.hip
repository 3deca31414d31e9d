// vrt_rays.hip -- ray generation for caller-side cameras: a hand-written HIP kernel for gfx950 (MI355X, CDNA4).
//
//   k_camera_rays   the rays of a W x H frame under one of three camera models -- main()'s pinhole with a field of view, an
//                   orthographic view, an equirectangular panorama -- into the two planes of 3 floats per ray that
//                   vrt_trace_rays and vrt_occluded_rays take (csrc/vrt_raygen.h is the definition, step by step in fp32)
//   k_camera_rays_offset   the same rays through (px + 0.5 + ox, py + 0.5 + oy): camera_ray_offset (vrt_camera_rays_offset)
//
// One lane per pixel, 64 consecutive pixels of a row per wave: a wave writes 768 contiguous bytes of each plane (three dword
// stores per plane at 12-byte stride, which the L2 merges into whole lines).  The kernel is a stream of 24 B per pixel; nothing
// in it is worth more than that.
#include "vrt_device_common.h"
#include "vrt_raygen.h"

namespace vrt {

__global__ __launch_bounds__(256) void k_camera_rays(const RayCamConsts k, const float* __restrict__ col, const float* __restrict__ row,
                                                     float* __restrict__ origins, float* __restrict__ dirs)
{
    const int px = (int)(blockIdx.x * 64u + (threadIdx.x & 63u)), py = (int)(blockIdx.y * 4u + (threadIdx.x >> 6));
    if (px >= k.W || py >= k.H) return;
    f3 o, d;
    camera_ray(k, col, row, px, py, o, d);
    const size_t i = ((size_t)py * (size_t)k.W + (size_t)px) * 3u;
    origins[i] = o.x; origins[i + 1] = o.y; origins[i + 2] = o.z;
    dirs[i] = d.x; dirs[i + 1] = d.y; dirs[i + 2] = d.z;
}

hipError_t launch_camera_rays(const RayCamConsts& k, const float* col, const float* row, float* origins, float* dirs, hipStream_t s)
{
    const dim3 grid((unsigned)((k.W + 63) / 64), (unsigned)((k.H + 3) / 4));
    hipLaunchKernelGGL(k_camera_rays, grid, dim3(256), 0, s, k, col, row, origins, dirs);
    return hipGetLastError();
}

// k_camera_rays_offset: the same stream for camera_ray_offset (vrt_camera_rays_offset); a kernel of its own, so that k_camera_rays
// stays as it is.  The two offsets travel in the kernel arguments; the panorama's are in its tables already.
__global__ __launch_bounds__(256) void k_camera_rays_offset(const RayCamConsts k, const float* __restrict__ col, const float* __restrict__ row,
                                                            const float ox, const float oy, float* __restrict__ origins, float* __restrict__ dirs)
{
    const int px = (int)(blockIdx.x * 64u + (threadIdx.x & 63u)), py = (int)(blockIdx.y * 4u + (threadIdx.x >> 6));
    if (px >= k.W || py >= k.H) return;
    f3 o, d;
    camera_ray_offset(k, col, row, ox, oy, px, py, o, d);
    const size_t i = ((size_t)py * (size_t)k.W + (size_t)px) * 3u;
    origins[i] = o.x; origins[i + 1] = o.y; origins[i + 2] = o.z;
    dirs[i] = d.x; dirs[i + 1] = d.y; dirs[i + 2] = d.z;
}

hipError_t launch_camera_rays_offset(const RayCamConsts& k, const float* col, const float* row, float ox, float oy, float* origins,
                                     float* dirs, hipStream_t s)
{
    const dim3 grid((unsigned)((k.W + 63) / 64), (unsigned)((k.H + 3) / 4));
    hipLaunchKernelGGL(k_camera_rays_offset, grid, dim3(256), 0, s, k, col, row, ox, oy, origins, dirs);
    return hipGetLastError();
}

} // namespace vrt
