// vrt_upsample.hip -- k_upsample for gfx950: temporal upsampling, a display-resolution history fed by jittered render-resolution
// frames (vrt_upsample).  What a pixel computes is upsample_pixel (vrt_upsample.h), the definition the tests restate; this file
// is the memory side.  An object of its own: no other stage's kernels see it.
//
//   k_upsample   one thread per DISPLAY pixel, one wave = 64 consecutive pixels of a display row, workgroups of 4 rows (as
//                k_reproject).
//
// Memory, per display pixel at scale s = TW / w: the current planes are w x h, so 24 / s^2 B of them come from HBM (colour 4,
// position 16, normal 4 per RENDER texel), but each texel is read by about s^2 lanes spread over up to three display rows --
// PLAIN loads, so that L2 keeps it for the waves of the rows below (a nontemporal load would fetch it from HBM once per row).
// The history is gathered with plain loads as in k_reproject, up to 4 x (16 + 8) B: a tap's surface texel is ONE 16-byte load,
// its colour is loaded only if the tap is valid, a tap of weight 0 not at all; a pixel that carries its history whole
// reads the nearest texel once more (16 + 8 B, in L2 from the tap loop).  Every output is touched once per frame and goes
// past the caches (nontemporal: 16 B per lane for the surface, 8 for color16 and motion, 4 for resolved): 36 B.  The
// pixel-independent constants travel in the kernel arguments (scalar registers).  No LDS, no scratch.
// Arithmetic: two projections, four IEEE divisions per pixel.
#include "vrt_device_common.h"
#include "vrt_upsample.h"

namespace vrt {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

__global__ __launch_bounds__(256) void k_upsample(const UpsampleParams p)
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
    upsample_pixel(p.k, X, Y, P4, N, c, p.hist_surface, p.hist_color, o);
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

hipError_t launch_upsample(const UpsampleParams& p, hipStream_t s)
{
    if (p.k.TWi <= 0 || p.k.THi <= 0 || p.k.wi <= 0 || p.k.hi <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_upsample, dim3((unsigned)((p.k.TWi + 63) / 64), (unsigned)((p.k.THi + 3) / 4)), dim3(256), 0, s, p);
    return hipGetLastError();
}

} // namespace vrt
