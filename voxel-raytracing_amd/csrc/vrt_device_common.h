// vrt_device_common.h -- what the device translation units (vrt_scene_build.hip, vrt_scene_edit.hip, vrt_device.hip,
// vrt_denoise.hip, vrt_post.hip) share beyond vrt_internal.h.  Not part of the public interface.
#pragma once

#include "vrt_internal.h"
#include "vrt_spec.h"

// cap of the dense scene's clearance fields (scene build; the edit kernels assert that vrt_edit.h states its regions for it)
#define VRT_DF_CAP 127      // >= 64: a 64-iteration AO ray that starts in the open is decided by its first look-up (trace_df_fast, any-hit)

namespace vrt {

// UNORM8 / SNORM8 code -> float: q0 = c * r, q = fma(fma(-D, q0, c), r, q0) with r = RN(1 / D) equals the IEEE quotient c / D
// for every one of the 256 codes (checked exhaustively in tests/test_denoise_decode.py): 3 VALU ops instead of ~11.
__device__ __forceinline__ float decode_unorm8(uint32_t c)
{
    const float r = 1.0f / 255.0f;
    float cf = (float)c, q0 = cf * r;
    return __builtin_fmaf(__builtin_fmaf(-255.0f, q0, cf), r, q0);
}
__device__ __forceinline__ float decode_snorm8(int32_t c)
{
    const float r = 1.0f / 127.0f;
    float cf = (float)c, q0 = cf * r;
    return fmaxf(__builtin_fmaf(__builtin_fmaf(-127.0f, q0, cf), r, q0), -1.0f);
}

// primary_dir with fewer instructions (K1; an IEEE division expands to ~11 VALU instructions, and ray generation has five):
//  * the two screen divisions by the 3-instruction sequence of screen_div_fast when the host found it exact for every
//    pixel centre of this screen size (P.fast_screen_div);
//  * normalize: the three divisions by the length share the reciprocal.  The instructions are those of the compiler's
//    expansion of x / l without v_div_scale / v_div_fixup, which do nothing when numerator and denominator are normal
//    numbers whose exponents differ by less than 96 and whose quotient is normal: guaranteed here for a whole wave by
//    2^-40 <= min |component| and length <= 2^40 (a component never exceeds the length by more than rounding).  Any other
//    wave -- zero components, huge or tiny camera vectors, NaN -- takes normalize3.
__device__ __forceinline__ f3 primary_v(const RayGenConsts& g, float crx, float cry, float crz, float rcp_w, float rcp_h,
                                        int fast_screen_div, int px, int py)
{
    float fx = (float)px + 0.5f, fy = (float)py + 0.5f;
    float qx, qy;
    if (fast_screen_div) { qx = screen_div_fast(fx, g.W, rcp_w); qy = screen_div_fast(fy, g.H, rcp_h); }
    else                 { qx = fx / g.W; qy = fy / g.H; }
    float sx = qx * 2.0f - 1.0f;
    float sy = qy * 2.0f - 1.0f;
    float vx = ((g.cd.x + sx * crx) + sy * g.planeV.x) + g.jx;
    float vy = ((g.cd.y + sx * cry) + sy * g.planeV.y) + g.jy;
    float vz = ((g.cd.z + sx * crz) + sy * g.planeV.z) + 0.0f;
    return mk3(vx, vy, vz);
}
// ... and its normalize()
__device__ __forceinline__ f3 primary_normalize(const f3 v)
{
    const float vx = v.x, vy = v.y, vz = v.z;
    const float l = len3(v);
    const float lo = __builtin_fminf(__builtin_fminf(__builtin_fabsf(vx), __builtin_fabsf(vy)), __builtin_fabsf(vz));
    const bool tame = lo >= 0x1p-40f && l <= 0x1p40f;
    if (__ballot(!tame) != 0ull) return normalize3(v);
    const float r0 = __builtin_amdgcn_rcpf(l);
    const float r = __builtin_fmaf(__builtin_fmaf(-l, r0, 1.0f), r0, r0);
    f3 o;
    { float q = vx * r; q = __builtin_fmaf(__builtin_fmaf(-l, q, vx), r, q); o.x = __builtin_fmaf(__builtin_fmaf(-l, q, vx), r, q); }
    { float q = vy * r; q = __builtin_fmaf(__builtin_fmaf(-l, q, vy), r, q); o.y = __builtin_fmaf(__builtin_fmaf(-l, q, vy), r, q); }
    { float q = vz * r; q = __builtin_fmaf(__builtin_fmaf(-l, q, vz), r, q); o.z = __builtin_fmaf(__builtin_fmaf(-l, q, vz), r, q); }
    return o;
}

// Row mapping shared by the denoiser and the strip copy kernels: local row index -> frame row.
__device__ __forceinline__ int strip_row(const ShardMap& sh, int extend, int r, int H)
{
    int per = sh.strip_rows + 2 * extend;
    int k = r / per, j = r % per;
    int g = k * sh.nranks + sh.rank;
    int y = g * sh.strip_rows - extend + j;
    int end = (g + 1) * sh.strip_rows; if (end > H) end = H;
    if (y < 0 || y >= end + extend || y >= H) return -1;
    return y;
}

} // namespace vrt
