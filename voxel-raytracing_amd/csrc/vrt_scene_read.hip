// vrt_scene_read.hip -- scene read-back kernels for gfx950 (vrt_scene_read_box, vrt_scene_list_box) and their launchers.
// vrt_scene_read.h has the definitions: box index, record, segments, and why the listing needs no sort.
//   k_read_box<BRICK>      the ids of a box, x fastest, into a staging buffer (bricks: gathered through the packed entries)
//   k_list_bricks          bricks: how many bricks the box meets are occupied (one block; a box over empty bricks ends here)
//   k_list_count<BRICK>    one wave per segment of 64 voxels: the ballot of id != 0, its population count per segment
//   k_list_scan            one block: the exclusive scan of the segments' counts in place, the total behind them
//   k_list_scatter<BRICK>  the same ballot again; a lane's record goes to its segment's first record + the lanes below it
// An empty brick costs the 32-bit load of the low half of its entry and nothing else: its pool is never touched.
#include "vrt_device_common.h"
#define VRT_SCENE_READ_LAUNCHERS
#include "vrt_scene_read.h"

namespace vrt {

// blockIdx.y / .z: y and z within the box
template <bool BRICK>
__global__ __launch_bounds__(256) void k_read_box(const ReadBox B, uint8_t* __restrict__ ids)
{
    const uint32_t bx = blockIdx.x * blockDim.x + threadIdx.x;
    if (bx >= B.size[0]) return;
    const uint32_t by = blockIdx.y, bz = blockIdx.z;
    ids[read_box_index(bx, by, bz, B.size)] = (uint8_t)read_voxel<BRICK>(B, B.lo[0] + (int)bx, B.lo[1] + (int)by, B.lo[2] + (int)bz);
}

// the bricks the box meets: t_lo .. t_lo + t_n per axis
struct ListBricks { int t_lo[3], t_n[3]; };

__device__ __host__ inline ListBricks list_bricks_of(const ReadBox& B)
{
    ListBricks t;
    for (int a = 0; a < 3; a++) {
        t.t_lo[a] = B.lo[a] >> 3;
        t.t_n[a] = ((B.lo[a] + (int)B.size[a] - 1) >> 3) - t.t_lo[a] + 1;
    }
    return t;
}

__global__ __launch_bounds__(256) void k_list_bricks(const ReadBox B, const ListBricks T, uint32_t* __restrict__ occupied)
{
    __shared__ uint32_t part[256];
    const uint32_t n = (uint32_t)T.t_n[0] * (uint32_t)T.t_n[1] * (uint32_t)T.t_n[2];
    uint32_t mine = 0;
    for (uint32_t t = threadIdx.x; t < n; t += 256u) {
        const int bx = T.t_lo[0] + (int)(t % (uint32_t)T.t_n[0]), by = T.t_lo[1] + (int)((t / (uint32_t)T.t_n[0]) % (uint32_t)T.t_n[1]);
        const int bz = T.t_lo[2] + (int)(t / ((uint32_t)T.t_n[0] * (uint32_t)T.t_n[1]));
        const size_t pc = (size_t)(bx + 1) + ((size_t)(by + 1) + (size_t)(bz + 1) * (size_t)B.pby) * (size_t)B.pbx;
        const uint32_t ptr = ((const uint32_t*)B.bentry)[2u * pc] & 0xFFFFFFu;
        mine += (ptr != 0u && ptr <= B.bcap) ? 1u : 0u;
    }
    part[threadIdx.x] = mine;
    __syncthreads();
    for (uint32_t w = 128u; w > 0u; w >>= 1) {
        if (threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0u) *occupied = part[0];
}

// segment g of the box -> the id of this lane's voxel (0 beyond the row's end); false: no such segment (wave-uniform)
template <bool BRICK>
__device__ __forceinline__ bool list_lane(const ReadBox& B, uint32_t g, uint32_t lane, uint32_t& bx, uint32_t& by, uint32_t& bz, uint32_t& id)
{
    const uint32_t spr = list_segments_per_row(B.size[0]);
    if (g >= spr * B.size[1] * B.size[2]) return false;
    const uint32_t row = g / spr;
    bx = (g - row * spr) * VRT_LIST_SEGMENT + lane;
    bz = row / B.size[1];
    by = row - bz * B.size[1];
    id = bx < B.size[0] ? read_voxel<BRICK>(B, B.lo[0] + (int)bx, B.lo[1] + (int)by, B.lo[2] + (int)bz) : 0u;
    return true;
}

// four waves per block, a segment each
template <bool BRICK>
__global__ __launch_bounds__(256) void k_list_count(const ReadBox B, uint32_t* __restrict__ work)
{
    const uint32_t lane = threadIdx.x & 63u, g = blockIdx.x * 4u + (threadIdx.x >> 6);
    uint32_t bx, by, bz, id;
    if (!list_lane<BRICK>(B, g, lane, bx, by, bz, id)) return;
    const uint64_t mask = __ballot(id != 0u);
    if (lane == 0u) work[g] = (uint32_t)__popcll(mask);
}

// work[0 .. n) -> its exclusive scan, work[n] = the total.  One block of 1024 threads: a thread sums a run of consecutive
// segments, the runs' sums are scanned in LDS, the thread rewrites its run.
__global__ __launch_bounds__(1024) void k_list_scan(uint32_t* __restrict__ work, uint32_t n)
{
    __shared__ uint32_t sums[1024];
    const uint32_t per = (n + 1023u) / 1024u;
    const uint32_t a = threadIdx.x * per < n ? threadIdx.x * per : n, b = a + per < n ? a + per : n;
    uint32_t sum = 0;
    for (uint32_t i = a; i < b; i++) sum += work[i];
    sums[threadIdx.x] = sum;
    __syncthreads();
    for (uint32_t d = 1u; d < 1024u; d <<= 1) {                 // inclusive scan of the 1024 sums
        const uint32_t v = threadIdx.x >= d ? sums[threadIdx.x - d] : 0u;
        __syncthreads();
        sums[threadIdx.x] += v;
        __syncthreads();
    }
    uint32_t run = sums[threadIdx.x] - sum;                     // records in front of this thread's run
    for (uint32_t i = a; i < b; i++) { const uint32_t c = work[i]; work[i] = run; run += c; }
    if (threadIdx.x == 1023u) work[n] = sums[1023];
}

template <bool BRICK>
__global__ __launch_bounds__(256) void k_list_scatter(const ReadBox B, const uint32_t* __restrict__ work, uint32_t total, uint32_t* __restrict__ records)
{
    const uint32_t lane = threadIdx.x & 63u, g = blockIdx.x * 4u + (threadIdx.x >> 6);
    uint32_t bx, by, bz, id;
    if (!list_lane<BRICK>(B, g, lane, bx, by, bz, id)) return;
    const uint64_t mask = __ballot(id != 0u);
    if (id == 0u) return;
    const uint32_t at = work[g] + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
    if (at < total) records[at] = list_record(bx, by, bz, id);
}

hipError_t launch_read_box(const ReadBox& b, uint8_t* ids, hipStream_t s)
{
    const dim3 grid((b.size[0] + 255u) / 256u, b.size[1], b.size[2]);
    if (b.vox) hipLaunchKernelGGL(k_read_box<false>, grid, dim3(256), 0, s, b, ids);
    else       hipLaunchKernelGGL(k_read_box<true>, grid, dim3(256), 0, s, b, ids);
    return hipGetLastError();
}

hipError_t launch_list_bricks(const ReadBox& b, uint32_t* occupied, hipStream_t s)
{
    hipLaunchKernelGGL(k_list_bricks, dim3(1), dim3(256), 0, s, b, list_bricks_of(b), occupied);
    return hipGetLastError();
}

uint32_t list_segments(const ReadBox& b) { return list_segments_per_row(b.size[0]) * b.size[1] * b.size[2]; }

hipError_t launch_list_count(const ReadBox& b, uint32_t* work, hipStream_t s)
{
    const uint32_t n = list_segments(b);
    if (b.vox) hipLaunchKernelGGL(k_list_count<false>, dim3((n + 3u) / 4u), dim3(256), 0, s, b, work);
    else       hipLaunchKernelGGL(k_list_count<true>, dim3((n + 3u) / 4u), dim3(256), 0, s, b, work);
    return launch_list_scan(work, n, s);
}

hipError_t launch_list_scan(uint32_t* work, uint32_t n, hipStream_t s)
{
    hipLaunchKernelGGL(k_list_scan, dim3(1), dim3(1024), 0, s, work, n);
    return hipGetLastError();
}

hipError_t launch_list_scatter(const ReadBox& b, const uint32_t* work, uint32_t total, uint32_t* records, hipStream_t s)
{
    const uint32_t n = list_segments(b);
    if (b.vox) hipLaunchKernelGGL(k_list_scatter<false>, dim3((n + 3u) / 4u), dim3(256), 0, s, b, work, total, records);
    else       hipLaunchKernelGGL(k_list_scatter<true>, dim3((n + 3u) / 4u), dim3(256), 0, s, b, work, total, records);
    return hipGetLastError();
}

} // namespace vrt
