// vrt_brush.hip -- scene brushes and stamps for gfx950 (vrt_scene_brush, vrt_scene_stamp): the kernels between the read-back's
// gather and the edits' write.  vrt_brush.h has the definitions (shapes, modes, orientations), vrt_brush_launch.h the job.
//   k_brush_extent<FORM>   one wave per segment of 64 voxels of a row of the clipped bounds (the segments of vrt_scene_read.h): a
//                          lane reads its voxel, evaluates what it becomes, the wave ballots new != old.  A wave with an empty
//                          ballot is done; the others add their count, bounds and written ids to the block's record in LDS (one
//                          lane each), and a block with any change adds its record to the launch's with one set of atomics.
//   k_brush_compose<FORM>  the same evaluation over the tight box of the changed voxels: the box's new ids into the edits' scratch
//                          in read_box_index order, which is what k_edit_write and bedit_box_id read.
// FORM: the three shapes, and a stamp (the source box gathered by k_read_box, indexed through stamp_source).  A dense scene and
// a brick scene share the kernels (a wave-uniform branch on the view): an empty brick costs the 32-bit load of the low half of
// its entry and reads no pool.  Ordinary vector loads and stores; no inline assembly.
#include "vrt_device_common.h"
#include "vrt_brush_launch.h"

namespace vrt {

__device__ __forceinline__ uint32_t brush_read_voxel(const ReadBox& B, int x, int y, int z)
{
    if (B.vox) return B.vox[(size_t)x + ((size_t)y + (size_t)z * (size_t)B.H) * (size_t)B.W];
    const size_t pc = (size_t)((x >> 3) + 1) + ((size_t)((y >> 3) + 1) + (size_t)((z >> 3) + 1) * (size_t)B.pby) * (size_t)B.pbx;
    const uint32_t ptr = ((const uint32_t*)B.bentry)[2u * pc] & 0xFFFFFFu;          // the entry's low word: pointer | open bits << 24
    if (ptr == 0u || ptr > B.bcap) return 0u;
    return B.bpool[(size_t)(ptr - 1u) * 512u + (size_t)((x & 7) | ((y & 7) << 3) | ((z & 7) << 6))];
}

// what voxel (x, y, z), which lies inside J.box, becomes
template <int FORM>
__device__ __forceinline__ uint32_t brush_new(const BrushJob& J, int x, int y, int z, uint32_t old)
{
    if (FORM == VRT_BRUSH_FORM_STAMP) {
        uint32_t s[3];
        stamp_source(J.orient, J.src_size, (uint32_t)(x - J.dst_lo[0]), (uint32_t)(y - J.dst_lo[1]), (uint32_t)(z - J.dst_lo[2]), s);
        return stamp_value(old, J.stage[read_box_index(s[0], s[1], s[2], J.src_size)], J.skip_empty != 0u);
    }
    return brush_inside(FORM, J.p, x, y, z) ? brush_value(J.mode, old, J.id, J.match) : old;
}

// segment g of J.box -> this lane's voxel, its id and what it becomes; in_row: the lane lies in the row.  false: no such segment
// (wave-uniform)
template <int FORM>
__device__ __forceinline__ bool brush_lane(const BrushJob& J, uint32_t g, uint32_t lane, uint32_t& bx, uint32_t& by, uint32_t& bz, bool& in_row,
                                           uint32_t& old, uint32_t& nw)
{
    const ReadBox& B = J.box;
    const uint32_t spr = list_segments_per_row(B.size[0]);
    if (g >= spr * B.size[1] * B.size[2]) return false;
    const uint32_t row = g / spr;
    bx = (g - row * spr) * VRT_LIST_SEGMENT + lane;
    bz = row / B.size[1];
    by = row - bz * B.size[1];
    in_row = bx < B.size[0];
    old = 0u; nw = 0u;
    if (in_row) {
        const int x = B.lo[0] + (int)bx, y = B.lo[1] + (int)by, z = B.lo[2] + (int)bz;
        old = brush_read_voxel(B, x, y, z);
        nw = brush_new<FORM>(J, x, y, z, old);
    }
    return true;
}

// four waves per block, a segment each
template <int FORM>
__global__ __launch_bounds__(256) void k_brush_extent(const BrushJob J, BrushRecord* __restrict__ rec)
{
    __shared__ uint32_t s_count;
    __shared__ int32_t s_mn[3], s_mx[3];
    __shared__ uint32_t s_ids[8];
    if (threadIdx.x < 8u) s_ids[threadIdx.x] = 0u;
    if (threadIdx.x < 3u) { s_mn[threadIdx.x] = INT32_MAX; s_mx[threadIdx.x] = INT32_MIN; }
    if (threadIdx.x == 0u) s_count = 0u;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, g = blockIdx.x * 4u + (threadIdx.x >> 6);
    uint32_t bx, by, bz, old, nw;
    bool in_row;
    if (brush_lane<FORM>(J, g, lane, bx, by, bz, in_row, old, nw)) {
        const bool changed = in_row && nw != old;
        const uint64_t mask = __ballot(changed);
        if (mask != 0ull) {
            // a stamp writes the ids of its source; a brush writes one id
            if (FORM == VRT_BRUSH_FORM_STAMP && changed) atomicOr(&s_ids[nw >> 5], 1u << (nw & 31u));
            if (lane == 0u) {
                const int x0 = J.box.lo[0] + (int)(bx + (uint32_t)__builtin_ctzll(mask)), x1 = J.box.lo[0] + (int)(bx + 63u - (uint32_t)__builtin_clzll(mask));
                const int y = J.box.lo[1] + (int)by, z = J.box.lo[2] + (int)bz;
                atomicAdd(&s_count, (uint32_t)__popcll(mask));
                atomicMin(&s_mn[0], x0); atomicMax(&s_mx[0], x1);
                atomicMin(&s_mn[1], y);  atomicMax(&s_mx[1], y);
                atomicMin(&s_mn[2], z);  atomicMax(&s_mx[2], z);
                if (FORM != VRT_BRUSH_FORM_STAMP) atomicOr(&s_ids[J.id >> 5], 1u << (J.id & 31u));
            }
        }
    }
    __syncthreads();
    if (s_count == 0u) return;
    if (threadIdx.x == 0u) atomicAdd(&rec->changed, (unsigned long long)s_count);
    if (threadIdx.x < 3u) { atomicMin(&rec->mn[threadIdx.x], s_mn[threadIdx.x]); atomicMax(&rec->mx[threadIdx.x], s_mx[threadIdx.x]); }
    if (threadIdx.x < 8u && s_ids[threadIdx.x] != 0u) atomicOr(&rec->ids[threadIdx.x], s_ids[threadIdx.x]);
}

template <int FORM>
__global__ __launch_bounds__(256) void k_brush_compose(const BrushJob J, uint8_t* __restrict__ ids)
{
    const uint32_t lane = threadIdx.x & 63u, g = blockIdx.x * 4u + (threadIdx.x >> 6);
    uint32_t bx, by, bz, old, nw;
    bool in_row;
    if (!brush_lane<FORM>(J, g, lane, bx, by, bz, in_row, old, nw)) return;
    if (in_row) ids[read_box_index(bx, by, bz, J.box.size)] = (uint8_t)nw;
}

static uint32_t brush_blocks(const BrushJob& j)
{
    return (list_segments_per_row(j.box.size[0]) * j.box.size[1] * j.box.size[2] + 3u) / 4u;
}

hipError_t launch_brush_extent(const BrushJob& j, BrushRecord* rec, hipStream_t s)
{
    const dim3 grid(brush_blocks(j)), block(256);
    switch (j.form) {
    case VRT_BRUSH_SHAPE_BOX:       hipLaunchKernelGGL(k_brush_extent<VRT_BRUSH_SHAPE_BOX>, grid, block, 0, s, j, rec); break;
    case VRT_BRUSH_SHAPE_ELLIPSOID: hipLaunchKernelGGL(k_brush_extent<VRT_BRUSH_SHAPE_ELLIPSOID>, grid, block, 0, s, j, rec); break;
    case VRT_BRUSH_SHAPE_CAPSULE:   hipLaunchKernelGGL(k_brush_extent<VRT_BRUSH_SHAPE_CAPSULE>, grid, block, 0, s, j, rec); break;
    case VRT_BRUSH_FORM_STAMP:      hipLaunchKernelGGL(k_brush_extent<VRT_BRUSH_FORM_STAMP>, grid, block, 0, s, j, rec); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_brush_compose(const BrushJob& j, uint8_t* ids, hipStream_t s)
{
    const dim3 grid(brush_blocks(j)), block(256);
    switch (j.form) {
    case VRT_BRUSH_SHAPE_BOX:       hipLaunchKernelGGL(k_brush_compose<VRT_BRUSH_SHAPE_BOX>, grid, block, 0, s, j, ids); break;
    case VRT_BRUSH_SHAPE_ELLIPSOID: hipLaunchKernelGGL(k_brush_compose<VRT_BRUSH_SHAPE_ELLIPSOID>, grid, block, 0, s, j, ids); break;
    case VRT_BRUSH_SHAPE_CAPSULE:   hipLaunchKernelGGL(k_brush_compose<VRT_BRUSH_SHAPE_CAPSULE>, grid, block, 0, s, j, ids); break;
    case VRT_BRUSH_FORM_STAMP:      hipLaunchKernelGGL(k_brush_compose<VRT_BRUSH_FORM_STAMP>, grid, block, 0, s, j, ids); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

} // namespace vrt
