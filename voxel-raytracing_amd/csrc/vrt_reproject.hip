// vrt_reproject.hip -- k_reproject for gfx950: temporal reprojection of the history under a moving camera (vrt_reproject).
// What a pixel computes is reproject_pixel (vrt_reproject.h), the definition the tests restate; this file is the memory
// side.  An object of its own: no other stage's kernels see it.
//
//   k_reproject   one thread per pixel, one wave = 64 consecutive pixels of a row, workgroups of 4 rows (as k_blit).
//
// Memory, per pixel: 24 B of current planes in (colour 4, position 16, normal 4), up to 4 x (16 + 8) B of history gathered --
// about 24 B from HBM, neighbouring lanes' taps being neighbouring texels, the rest from L2 -- and 36 B out (color16 8,
// surface 16, resolved 4, motion 8).  The current planes and every output are touched once per frame and go past the caches
// (nontemporal, 16 B per lane for position / surface: a wave's access is 1 KiB of consecutive bytes); the history is read
// with plain loads, so that the up to four waves that touch a texel find it in L2.  A tap's surface texel -- position, normal
// and count -- is ONE 16-byte load; its colour is loaded only if the tap is valid, a tap of weight 0 not at all.  The
// pixel-independent constants travel in the kernel arguments (scalar registers).  No LDS, no scratch.
#include "vrt_device_common.h"
#include "vrt_reproject.h"

namespace vrt {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

__global__ __launch_bounds__(256) void k_reproject(const ReprojectParams p)
{
    const int px = blockIdx.x * 64 + (threadIdx.x & 63), py = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (px >= p.k.Wi || py >= p.k.Hi) return;
    const size_t i = (size_t)py * (size_t)p.k.Wi + (size_t)px;
    const uint32_t c = __builtin_nontemporal_load(p.color8 + i);
    const uint32_t N = __builtin_nontemporal_load(p.normal8 + i);
    const u32x4 pv = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p.position) + i);
    rp_u4 P4; P4.x = pv.x; P4.y = pv.y; P4.z = pv.z; P4.w = pv.w;
    ReprojectPixel o;
    reproject_pixel(p.k, px, py, P4, N, c, p.hist_surface, p.hist_color, o);
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

hipError_t launch_reproject(const ReprojectParams& p, hipStream_t s)
{
    if (p.k.Wi <= 0 || p.k.Hi <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_reproject, dim3((unsigned)((p.k.Wi + 63) / 64), (unsigned)((p.k.Hi + 3) / 4)), dim3(256), 0, s, p);
    return hipGetLastError();
}

} // namespace vrt
