// vrt_voxelize.hip -- mesh voxelization for gfx950 (vrt_scene_voxelize): a triangle mesh becomes a coverage mask on the device,
// which the edits take as they take a flood's region.  vrt_voxelize.h has the definition, the masks' layout and every bound,
// vrt_voxelize_launch.h the job.
//   k_vox_surface   one wave per work item (triangle, slab of rows of its clipped box).  The triangle is wave-uniform: vertices,
//                   edges, normal and radii are set up once per wave.  Per row (y, z) the five axes that depend on (y, z) only
//                   decide for the whole wave (vox_row_meets); a row they reject costs no per-lane work.  Otherwise 64 lanes
//                   test 64 x-consecutive voxels aligned to the mask word (vox_lane_meets), one ballot, and one lane does one
//                   64-bit atomicOr when the ballot is not empty.
//   k_vox_cross     one wave per item (triangle, slab of columns of its clipped yz-box), a lane per column: rule (a), then the
//                   length of the prefix of the row that satisfies (b) (vox_cross_count: one division, no loop over x), then
//                   one 64-bit atomicXor of that bit of the row's toggle word.
//   k_vox_scan      a thread per row: inside() from the toggle bits by in-word shifts and a carry from word to word
//                   (vox_scan_word), ORed into the coverage mask.
//   k_vox_extent    k_flood_extent with "inside" = the coverage bit and value = brush_value: the covered count, the changed
//                   count, the tight box, the ids written.
//   k_vox_compose   k_flood_compose likewise: the tight box's new ids into the edits' scratch in read_box_index order.
// A dense scene and a brick scene share the kernels (a wave-uniform branch on the view).  No wave waits for another.  Ordinary
// vector loads and stores, wave votes, atomics on the masks' words; no inline assembly.
#include "vrt_device_common.h"
#include "vrt_voxelize_launch.h"

namespace vrt {

__device__ __forceinline__ uint32_t vox_read_voxel(const ReadBox& B, int x, int y, int z)
{
    if (B.vox) return B.vox[(size_t)x + ((size_t)y + (size_t)z * (size_t)B.H) * (size_t)B.W];
    const size_t pc = (size_t)((x >> 3) + 1) + ((size_t)((y >> 3) + 1) + (size_t)((z >> 3) + 1) * (size_t)B.pby) * (size_t)B.pbx;
    const uint32_t ptr = ((const uint32_t*)B.bentry)[2u * pc] & 0xFFFFFFu;          // the entry's low word: pointer | open bits << 24
    if (ptr == 0u || ptr > B.bcap) return 0u;
    return B.bpool[(size_t)(ptr - 1u) * 512u + (size_t)((x & 7) | ((y & 7) << 3) | ((z & 7) << 6))];
}

// the item's triangle, set up (wave-uniform: every lane does the same loads and arithmetic)
__device__ __forceinline__ void vox_load_tri(const VoxJob& J, uint32_t tri, VoxTri& T)
{
    const uint32_t ia = J.triangles[3u * (size_t)tri], ib = J.triangles[3u * (size_t)tri + 1u], ic = J.triangles[3u * (size_t)tri + 2u];
    vox_tri_setup(J.vertices + 3u * (size_t)ia, J.vertices + 3u * (size_t)ib, J.vertices + 3u * (size_t)ic, T);
}

// four waves per block, an item each
__global__ __launch_bounds__(256) void k_vox_surface(const VoxJob J, const VoxItem* __restrict__ items, uint32_t nitems)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t g = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    if (g >= nitems) return;
    const VoxItem it = items[g];
    VoxTri T;
    vox_load_tri(J, it.tri, T);
    int32_t lo[3], hi[3];
    if (!vox_tri_box(T, false, J.clo, J.csize, lo, hi)) return;
    const uint32_t ny = (uint32_t)(hi[1] - lo[1] + 1), nz = (uint32_t)(hi[2] - lo[2] + 1);
    const uint32_t w0 = (uint32_t)(lo[0] - J.clo[0]) >> 6, w1 = (uint32_t)(hi[0] - J.clo[0]) >> 6, wpr = vox_cover_words(J.csize[0]);
    const uint32_t end = it.first + it.count < ny * nz ? it.first + it.count : ny * nz;
    for (uint32_t r = it.first; r < end; r++) {
        const uint32_t rz = r / ny, ry = r - rz * ny;
        const int32_t y = lo[1] + (int32_t)ry, z = lo[2] + (int32_t)rz, cy = vox_centre(y), cz = vox_centre(z);
        if (!vox_row_meets(T, cy, cz)) continue;                   // (wave-uniform)
        const size_t row = vox_row_index((uint32_t)(y - J.clo[1]), (uint32_t)(z - J.clo[2]), J.csize);
        for (uint32_t w = w0; w <= w1; w++) {
            const int32_t x = J.clo[0] + (int32_t)(w * 64u + lane);
            const bool hit = x >= lo[0] && x <= hi[0] && vox_lane_meets(T, vox_centre(x), cy, cz);
            const uint64_t m = __ballot(hit);
            if (m != 0ull && lane == 0u) atomicOr(&J.cover[row * wpr + w], (unsigned long long)m);
        }
    }
}

// four waves per block, an item each; a lane per column
__global__ __launch_bounds__(256) void k_vox_cross(const VoxJob J, const VoxItem* __restrict__ items, uint32_t nitems)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t g = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    if (g >= nitems) return;
    const VoxItem it = items[g];
    VoxTri T;
    vox_load_tri(J, it.tri, T);
    int32_t lo[3], hi[3];
    if (!vox_tri_box(T, true, J.clo, J.csize, lo, hi)) return;
    const int s = vox_cross_sign(T);
    const uint32_t ny = (uint32_t)(hi[1] - lo[1] + 1), nz = (uint32_t)(hi[2] - lo[2] + 1), tw = vox_toggle_words(J.csize[0]);
    const uint32_t end = it.first + it.count < ny * nz ? it.first + it.count : ny * nz;
    for (uint32_t c = it.first + lane; c < end; c += 64u) {
        const uint32_t rz = c / ny, ry = c - rz * ny;
        const int32_t y = lo[1] + (int32_t)ry, z = lo[2] + (int32_t)rz, cy = vox_centre(y), cz = vox_centre(z);
        if (!vox_column_inside(T, s, cy, cz)) continue;
        const uint32_t k = vox_cross_count(T, s, J.clo[0], J.csize[0], cy, cz);
        if (k == 0u) continue;
        const size_t row = vox_row_index((uint32_t)(y - J.clo[1]), (uint32_t)(z - J.clo[2]), J.csize);
        atomicXor(&J.toggle[row * tw + (k >> 6)], 1ull << (k & 63u));
    }
}

// a thread per row of the clipped bounds
__global__ __launch_bounds__(256) void k_vox_scan(const VoxJob J)
{
    const uint32_t rows = J.csize[1] * J.csize[2], row = blockIdx.x * 256u + threadIdx.x;
    if (row >= rows) return;
    const uint32_t tw = vox_toggle_words(J.csize[0]), wpr = vox_cover_words(J.csize[0]);
    uint64_t carry = 0ull;
    for (uint32_t w = tw; w-- > 0u;) {
        uint64_t in = vox_scan_word(J.toggle[(size_t)row * tw + w], &carry);
        if (w >= wpr) continue;
        in &= vox_word_valid(w, J.csize[0]);
        if (in != 0ull) J.cover[(size_t)row * wpr + w] |= (unsigned long long)in;       // the row is this thread's alone
    }
}

// segment g of J.box -> this lane's offset in the box; in_row: the lane lies in the row.  false: no such segment (wave-uniform)
__device__ __forceinline__ bool vox_lane(const ReadBox& B, uint32_t g, uint32_t lane, uint32_t& bx, uint32_t& by, uint32_t& bz, bool& in_row)
{
    const uint32_t spr = list_segments_per_row(B.size[0]);
    if (g >= spr * B.size[1] * B.size[2]) return false;
    const uint32_t row = g / spr;
    bx = (g - row * spr) * VRT_LIST_SEGMENT + lane;
    bz = row / B.size[1];
    by = row - bz * B.size[1];
    in_row = bx < B.size[0];
    return true;
}

// this lane's coverage bit; (bx, by, bz) is an offset in J.box, which lies inside the clipped bounds
__device__ __forceinline__ bool vox_covered(const VoxJob& J, uint32_t bx, uint32_t by, uint32_t bz)
{
    const uint32_t rx = (uint32_t)(J.box.lo[0] - J.clo[0]) + bx, ry = (uint32_t)(J.box.lo[1] - J.clo[1]) + by, rz = (uint32_t)(J.box.lo[2] - J.clo[2]) + bz;
    return ((J.cover[vox_row_index(ry, rz, J.csize) * vox_cover_words(J.csize[0]) + (rx >> 6)] >> (rx & 63u)) & 1ull) != 0ull;
}

// four waves per block, a segment each; J.box is the clipped bounds
__global__ __launch_bounds__(256) void k_vox_extent(const VoxJob J, VoxRecord* __restrict__ rec)
{
    __shared__ uint32_t s_covered, s_count;
    __shared__ int32_t s_mn[3], s_mx[3];
    if (threadIdx.x < 3u) { s_mn[threadIdx.x] = INT32_MAX; s_mx[threadIdx.x] = INT32_MIN; }
    if (threadIdx.x == 0u) { s_covered = 0u; s_count = 0u; }
    __syncthreads();
    const ReadBox& B = J.box;
    const uint32_t lane = threadIdx.x & 63u, g = blockIdx.x * 4u + (threadIdx.x >> 6);
    uint32_t bx, by, bz;
    bool in_row;
    if (vox_lane(B, g, lane, bx, by, bz, in_row)) {
        const bool inside = in_row && vox_covered(J, bx, by, bz);
        const uint64_t imask = __ballot(inside);
        if (imask != 0ull) {
            const int x = B.lo[0] + (int)bx, y = B.lo[1] + (int)by, z = B.lo[2] + (int)bz;
            bool changed = false;
            if (inside) {
                const uint32_t old = vox_read_voxel(B, x, y, z);
                changed = brush_value(J.mode, old, J.id, J.match) != old;
            }
            const uint64_t cmask = __ballot(changed);
            if (lane == 0u) {
                atomicAdd(&s_covered, (uint32_t)__popcll(imask));
                if (cmask != 0ull) {
                    atomicAdd(&s_count, (uint32_t)__popcll(cmask));
                    atomicMin(&s_mn[0], x + (int)__builtin_ctzll(cmask)); atomicMax(&s_mx[0], x + 63 - (int)__builtin_clzll(cmask));
                    atomicMin(&s_mn[1], y); atomicMax(&s_mx[1], y);
                    atomicMin(&s_mn[2], z); atomicMax(&s_mx[2], z);
                }
            }
        }
    }
    __syncthreads();
    if (s_covered == 0u) return;
    if (threadIdx.x == 0u) atomicAdd(&rec->covered, (unsigned long long)s_covered);
    if (s_count == 0u) return;
    if (threadIdx.x == 0u) { atomicAdd(&rec->edit.changed, (unsigned long long)s_count); atomicOr(&rec->edit.ids[J.id >> 5], 1u << (J.id & 31u)); }
    if (threadIdx.x < 3u) { atomicMin(&rec->edit.mn[threadIdx.x], s_mn[threadIdx.x]); atomicMax(&rec->edit.mx[threadIdx.x], s_mx[threadIdx.x]); }
}

// J.box is the tight box of the changed voxels
__global__ __launch_bounds__(256) void k_vox_compose(const VoxJob J, uint8_t* __restrict__ ids)
{
    const ReadBox& B = J.box;
    const uint32_t lane = threadIdx.x & 63u, g = blockIdx.x * 4u + (threadIdx.x >> 6);
    uint32_t bx, by, bz;
    bool in_row;
    if (!vox_lane(B, g, lane, bx, by, bz, in_row) || !in_row) return;
    const uint32_t old = vox_read_voxel(B, B.lo[0] + (int)bx, B.lo[1] + (int)by, B.lo[2] + (int)bz);
    ids[read_box_index(bx, by, bz, B.size)] = (uint8_t)(vox_covered(J, bx, by, bz) ? brush_value(J.mode, old, J.id, J.match) : old);
}

static uint32_t vox_blocks(const VoxJob& j)
{
    return (list_segments_per_row(j.box.size[0]) * j.box.size[1] * j.box.size[2] + 3u) / 4u;
}

hipError_t launch_vox_surface(const VoxJob& j, const VoxItem* items, uint32_t nitems, hipStream_t s)
{
    if (nitems == 0u) return hipSuccess;
    hipLaunchKernelGGL(k_vox_surface, dim3((nitems + 3u) / 4u), dim3(256), 0, s, j, items, nitems);
    return hipGetLastError();
}

hipError_t launch_vox_cross(const VoxJob& j, const VoxItem* items, uint32_t nitems, hipStream_t s)
{
    if (nitems == 0u) return hipSuccess;
    hipLaunchKernelGGL(k_vox_cross, dim3((nitems + 3u) / 4u), dim3(256), 0, s, j, items, nitems);
    return hipGetLastError();
}

hipError_t launch_vox_scan(const VoxJob& j, hipStream_t s)
{
    hipLaunchKernelGGL(k_vox_scan, dim3((j.csize[1] * j.csize[2] + 255u) / 256u), dim3(256), 0, s, j);
    return hipGetLastError();
}

hipError_t launch_vox_extent(const VoxJob& j, VoxRecord* rec, hipStream_t s)
{
    hipLaunchKernelGGL(k_vox_extent, dim3(vox_blocks(j)), dim3(256), 0, s, j, rec);
    return hipGetLastError();
}

hipError_t launch_vox_compose(const VoxJob& j, uint8_t* ids, hipStream_t s)
{
    hipLaunchKernelGGL(k_vox_compose, dim3(vox_blocks(j)), dim3(256), 0, s, j, ids);
    return hipGetLastError();
}

} // namespace vrt
