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
