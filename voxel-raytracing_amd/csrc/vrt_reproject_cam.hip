// vrt_reproject_cam.hip -- k_reproject_cam for gfx950: temporal reprojection under a ray camera (vrt_reproject_camera).
// What a pixel computes is reproject_cam_pixel (vrt_reproject_cam.h), the definition the tests restate; this file is the memory
// side, which is k_reproject's (vrt_reproject.hip) exactly.  An object of its own: no other stage's kernels see it.
//
//   k_reproject_cam<MODEL>   one instantiation per camera model (the pinhole's carries no transcendental code); one thread per
//                            pixel, one wave = 64 consecutive pixels of a row, workgroups of 4 rows.
//
// Memory, per pixel: 24 B of current planes in (colour 4, position 16, normal 4), up to 4 x (16 + 8) B of history gathered and
// 36 B out (color16 8, surface 16, resolved 4, motion 8).  The current planes and every output go past the caches (nontemporal,
// 16 B per lane for position / surface); the history is read with plain loads, so that the up to four waves that touch a texel
// find it in L2 -- the panorama's wrapped taps are the texels of the row's other end, which the waves there read anyway.  A tap's
// surface texel is ONE 16-byte load; its colour is loaded only if the tap is valid, a tap of weight 0 not at all.  The
// pixel-independent constants travel in the kernel arguments (scalar registers).  No LDS, no scratch.
//
// The panorama's atan2_spec runs under a divergent `front`: atan_unit's __ballot (vrt_spec.h) then sees the lanes that are in
// front only, and it decides nothing but whether the wave executes the reduced argument's division at all -- a lane takes the
// quotient only under its own `red`, and the quotient is div_spec of the lane's own operands either way.  No result depends on
// which lanes vote.
#include "vrt_device_common.h"
#include "vrt_reproject_cam.h"

namespace vrt {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

template <int MODEL>
__global__ __launch_bounds__(256) void k_reproject_cam(const ReprojectParams p)
{
    const int px = blockIdx.x * 64 + (threadIdx.x & 63), py = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (px >= p.k.Wi || py >= p.k.Hi) return;
    const size_t i = (size_t)py * (size_t)p.k.Wi + (size_t)px;
    const uint32_t c = __builtin_nontemporal_load(p.color8 + i);
    const uint32_t N = __builtin_nontemporal_load(p.normal8 + i);
    const u32x4 pv = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p.position) + i);
    rp_u4 P4; P4.x = pv.x; P4.y = pv.y; P4.z = pv.z; P4.w = pv.w;
    ReprojectPixel o;
    reproject_cam_pixel<MODEL>(p.k, px, py, P4, N, c, p.hist_surface, p.hist_color, o);
    u32x4 sv; sv.x = o.surface.x; sv.y = o.surface.y; sv.z = o.surface.z; sv.w = o.surface.w;
    u32x2 cv; cv.x = o.color16.x; cv.y = o.color16.y;
    __builtin_nontemporal_store(sv, reinterpret_cast<u32x4*>(p.out_surface) + i);
    __builtin_nontemporal_store(cv, reinterpret_cast<u32x2*>(p.out_color) + i);
    if (p.resolved8) __builtin_nontemporal_store(o.resolved, p.resolved8 + i);
    if (p.motion) {
        u32x2 mv; mv.x = __float_as_uint(o.mvx); mv.y = __float_as_uint(o.mvy);
        __builtin_nontemporal_store(mv, reinterpret_cast<u32x2*>(p.motion) + i);
    }
}

hipError_t launch_reproject_cam(int model, const ReprojectParams& p, hipStream_t s)
{
    if (p.k.Wi <= 0 || p.k.Hi <= 0) return hipSuccess;
    const dim3 grid((unsigned)((p.k.Wi + 63) / 64), (unsigned)((p.k.Hi + 3) / 4)), block(256);
    if (model == VRT_CAMERA_PERSPECTIVE) hipLaunchKernelGGL(k_reproject_cam<VRT_CAMERA_PERSPECTIVE>, grid, block, 0, s, p);
    else if (model == VRT_CAMERA_ORTHOGRAPHIC) hipLaunchKernelGGL(k_reproject_cam<VRT_CAMERA_ORTHOGRAPHIC>, grid, block, 0, s, p);
    else if (model == VRT_CAMERA_PANORAMA) hipLaunchKernelGGL(k_reproject_cam<VRT_CAMERA_PANORAMA>, grid, block, 0, s, p);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

} // namespace vrt
