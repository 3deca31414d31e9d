// vrt_upsample_cam.hip -- k_upsample_cam for gfx950: temporal upsampling under a ray camera (vrt_upsample_camera).  What a pixel
// computes is upsample_cam_pixel (vrt_upsample_cam.h), the definition the tests restate; this file is the memory side, which is
// k_upsample's (vrt_upsample.hip) exactly.  An object of its own: no other stage's kernels see it.
//
//   k_upsample_cam<MODEL>   one instantiation per camera model (the pinhole's and the orthographic one's carry no transcendental
//                           code); one thread per DISPLAY pixel, one wave = 64 consecutive pixels of a display row, workgroups of
//                           4 rows.
//
// Memory, per display pixel at scale s = TW / w, by k_upsample's accounting: 24 / s^2 B of current planes from HBM, read with
// PLAIN loads (about s^2 lanes over up to three display rows read a texel: L2 keeps it for the rows below); the history gathered
// with plain loads, up to 4 x (16 + 8) B -- a tap's surface texel is ONE 16-byte load, its colour is loaded only if the tap is
// valid, a tap of weight 0 not at all; a pixel that carries its history whole reads the nearest texel once more -- and 36 B out
// past the caches (nontemporal: surface 16, color16 8, motion 8, resolved 4).  The panorama's wrapped taps are the texels of the
// row's other end, which the waves there read anyway.  The pixel-independent constants travel in the kernel arguments (scalar
// registers).  No LDS, no scratch.
// Arithmetic: two projections per pixel -- four IEEE divisions, or for the panorama two atan2_spec / asin_spec pairs.
//
// The panorama's atan2_spec runs under a divergent `front`: atan_unit's __ballot (vrt_spec.h) then sees the lanes that are in
// front only, and it decides nothing but whether the wave executes the reduced argument's division at all (vrt_reproject_cam.hip).
// No result depends on which lanes vote.
#include "vrt_device_common.h"
#include "vrt_upsample_cam.h"

namespace vrt {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

template <int MODEL>
__global__ __launch_bounds__(256) void k_upsample_cam(const UpsampleParams p)
{
    const int X = blockIdx.x * 64 + (threadIdx.x & 63), Y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (X >= p.k.TWi || Y >= p.k.THi) return;
    int rx, ry;
    upsample_source(p.k, X, Y, rx, ry);                               // rx < w, ry < h
    const size_t j = (size_t)ry * (size_t)p.k.wi + (size_t)rx;
    const uint32_t c = p.color8[j];
    const uint32_t N = p.normal8[j];
    const u32x4 pv = *(reinterpret_cast<const u32x4*>(p.position) + j);
    rp_u4 P4; P4.x = pv.x; P4.y = pv.y; P4.z = pv.z; P4.w = pv.w;
    ReprojectPixel o;
    upsample_cam_pixel<MODEL>(p.k, X, Y, P4, N, c, p.hist_surface, p.hist_color, o);
    const size_t i = (size_t)Y * (size_t)p.k.TWi + (size_t)X;
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

hipError_t launch_upsample_cam(int model, const UpsampleParams& p, hipStream_t s)
{
    if (p.k.TWi <= 0 || p.k.THi <= 0 || p.k.wi <= 0 || p.k.hi <= 0) return hipSuccess;
    const dim3 grid((unsigned)((p.k.TWi + 63) / 64), (unsigned)((p.k.THi + 3) / 4)), block(256);
    if (model == VRT_CAMERA_PERSPECTIVE) hipLaunchKernelGGL(k_upsample_cam<VRT_CAMERA_PERSPECTIVE>, grid, block, 0, s, p);
    else if (model == VRT_CAMERA_ORTHOGRAPHIC) hipLaunchKernelGGL(k_upsample_cam<VRT_CAMERA_ORTHOGRAPHIC>, grid, block, 0, s, p);
    else if (model == VRT_CAMERA_PANORAMA) hipLaunchKernelGGL(k_upsample_cam<VRT_CAMERA_PANORAMA>, grid, block, 0, s, p);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

} // namespace vrt
