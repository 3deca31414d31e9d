// vrt_query_io.h -- how the query kernels (vrt_query.hip, vrt_query_seg.hip) move a wave's planes of three values per ray: through
// the wave's LDS, so that global memory only sees whole-dword, lane-contiguous instructions (vrt_query.hip says why).  Device only;
// one wave per workgroup, lds: the workgroup's 192 dwords.
#pragma once

#include "vrt_device_common.h"

namespace vrt {

// K dwords per ray: the wave's 64 * K dwords of `src` (rays base .. base + 63 of n) -> each lane's own K
template <int K>
__device__ __forceinline__ void wave_fetch(const uint32_t* __restrict__ src, uint32_t base, uint32_t n, uint32_t* lds, uint32_t lane, uint32_t (&out)[K])
{
    const uint32_t first = base * (uint32_t)K, total = n * (uint32_t)K;      // (n <= 2^28: no overflow)
#pragma unroll
    for (int q = 0; q < K; q++) {
        const uint32_t idx = first + (uint32_t)q * 64u + lane;
        lds[q * 64 + lane] = idx < total ? src[idx] : 0u;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; k++) out[k] = lds[lane * K + k];
    __syncthreads();
}

// ... and back: each lane's K dwords -> the wave's 64 * K dwords of `dst`; nothing is written past ray n - 1
template <int K>
__device__ __forceinline__ void wave_store(uint32_t* __restrict__ dst, uint32_t base, uint32_t n, uint32_t* lds, uint32_t lane, const uint32_t (&v)[K])
{
    const uint32_t first = base * (uint32_t)K, total = n * (uint32_t)K;
#pragma unroll
    for (int k = 0; k < K; k++) lds[lane * K + k] = v[k];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < K; q++) {
        const uint32_t idx = first + (uint32_t)q * 64u + lane;
        if (idx < total) dst[idx] = lds[q * 64 + lane];
    }
    __syncthreads();
}

// the normals, three bytes per ray: the wave's 192 bytes as 48 dwords (base * 3 is a multiple of 4; a plane that is not
// 4-byte aligned, and the last dword of a batch whose bytes end inside it, are stored byte by byte)
__device__ __forceinline__ void wave_store_normals(int8_t* __restrict__ dst, uint32_t base, uint32_t n, uint32_t* lds, uint32_t lane, bool live, int nx, int ny, int nz)
{
    if (((uintptr_t)dst & 3u) != 0u) {                        // (wave-uniform)
        if (live) { int8_t* d = dst + (size_t)(base + lane) * 3u; d[0] = (int8_t)nx; d[1] = (int8_t)ny; d[2] = (int8_t)nz; }
        return;
    }
    uint8_t* b = reinterpret_cast<uint8_t*>(lds);
    b[lane * 3 + 0] = (uint8_t)nx; b[lane * 3 + 1] = (uint8_t)ny; b[lane * 3 + 2] = (uint8_t)nz;
    __syncthreads();
    const uint32_t b0 = base * 3u + lane * 4u, total = n * 3u;
    if (lane < 48u) {
        if (b0 + 4u <= total) *reinterpret_cast<uint32_t*>(dst + b0) = lds[lane];
        else for (uint32_t j = 0; j < 4u; j++) if (b0 + j < total) dst[b0 + j] = (int8_t)b[lane * 4u + j];
    }
    __syncthreads();
}

} // namespace vrt
