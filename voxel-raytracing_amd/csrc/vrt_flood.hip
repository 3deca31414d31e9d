// vrt_flood.hip -- flood fill for gfx950 (vrt_scene_flood): select the connected region of a seed on the device, then hand it to
// the edits as a brush hands over its shape.  vrt_flood.h has the definition, the masks' layout and the wake-up invariant,
// vrt_flood_launch.h the job.
//   k_flood_pass         one wave per segment of 64 voxels of a row of the clipped bounds (the segments of vrt_scene_read.h): a
//                        lane reads its voxel and evaluates the predicate, the wave ballots; the ballot's eight bytes are the rows
//                        of eight tiles, stored by eight lanes.  The lane on the seed sets its bit of the reached mask and the
//                        flags of round 0 (flood_seed_tiles).
//   k_flood_round<CONN>  one wave (a block of 64) per tile, a lane per row (y, z).  A tile whose flag is clear is done at once.
//                        The others gather the tile's extended rows into LDS (flood_ext_row: the tile and its shell), relax
//                        them to a fixed point (flood_row_relax; a wave vote ends the loop), store the rows that gained bits and
//                        set the flags of the neighbour tiles that can see a gained bit (flood_wake_mask).
//   k_flood_extent       k_brush_extent with "inside" = the reached bit and value = the flood's id, plus the region's own count
//                        and bounds.
//   k_flood_compose      k_brush_compose likewise: the tight box's new ids into the edits' scratch in read_box_index order.
// A dense scene and a brick scene share the kernels (a wave-uniform branch on the view): an empty brick costs the 32-bit load of
// the low half of its entry and reads no pool.  No wave waits for another: a round is a launch, the loop over rounds is the
// host's.  Ordinary vector loads and stores, wave votes, LDS; no inline assembly.
#include "vrt_device_common.h"
#include "vrt_flood_launch.h"

namespace vrt {

__device__ __forceinline__ uint32_t flood_read_voxel(const ReadBox& B, int x, int y, int z)
{
    if (B.vox) return B.vox[(size_t)x + ((size_t)y + (size_t)z * (size_t)B.H) * (size_t)B.W];
    const size_t pc = (size_t)((x >> 3) + 1) + ((size_t)((y >> 3) + 1) + (size_t)((z >> 3) + 1) * (size_t)B.pby) * (size_t)B.pbx;
    const uint32_t ptr = ((const uint32_t*)B.bentry)[2u * pc] & 0xFFFFFFu;          // the entry's low word: pointer | open bits << 24
    if (ptr == 0u || ptr > B.bcap) return 0u;
    return B.bpool[(size_t)(ptr - 1u) * 512u + (size_t)((x & 7) | ((y & 7) << 3) | ((z & 7) << 6))];
}

// segment g of J.box -> this lane's offset in the box; in_row: the lane lies in the row.  false: no such segment (wave-uniform)
__device__ __forceinline__ bool flood_lane(const ReadBox& B, uint32_t g, uint32_t lane, uint32_t& seg, uint32_t& bx, uint32_t& by, uint32_t& bz, bool& in_row)
{
    const uint32_t spr = list_segments_per_row(B.size[0]);
    if (g >= spr * B.size[1] * B.size[2]) return false;
    const uint32_t row = g / spr;
    seg = g - row * spr;
    bx = seg * VRT_LIST_SEGMENT + lane;
    bz = row / B.size[1];
    by = row - bz * B.size[1];
    in_row = bx < B.size[0];
    return true;
}

// four waves per block, a segment each; J.box is the clipped bounds
__global__ __launch_bounds__(256) void k_flood_pass(const FloodJob J, uint32_t* __restrict__ act0, FloodRecord* __restrict__ rec)
{
    const ReadBox& B = J.box;
    const uint32_t lane = threadIdx.x & 63u, g = blockIdx.x * 4u + (threadIdx.x >> 6);
    uint32_t seg, bx, by, bz;
    bool in_row;
    if (!flood_lane(B, g, lane, seg, bx, by, bz, in_row)) return;
    const uint32_t seed_id = flood_read_voxel(B, J.seed[0], J.seed[1], J.seed[2]);
    bool pass = false;
    if (in_row) pass = flood_passes(J.match, flood_read_voxel(B, B.lo[0] + (int)bx, B.lo[1] + (int)by, B.lo[2] + (int)bz), seed_id);
    const uint64_t mask = __ballot(pass);
    const uint32_t tx = seg * 8u + lane;                          // lanes 0..7: the segment's eight tiles along x
    if (lane < 8u && tx < J.nt[0]) {
        const uint32_t byte = (uint32_t)(mask >> (8u * lane)) & 0xFFu;
        if (byte != 0u) J.passable[flood_tile_index(tx, by >> 3, bz >> 3, J.nt) * VRT_FLOOD_TILE_BYTES + ((by & 7u) | ((bz & 7u) << 3))] = (uint8_t)byte;
    }
    if (in_row && B.lo[0] + (int)bx == J.seed[0] && B.lo[1] + (int)by == J.seed[1] && B.lo[2] + (int)bz == J.seed[2]) {
        rec->seed_id = seed_id;
        if (pass) {
            J.reached[flood_mask_byte(bx, by, bz, J.nt)] = (uint8_t)(1u << flood_mask_bit(bx));
            const uint32_t tiles = flood_seed_tiles(J.connectivity, bx, by, bz);
            for (uint32_t o = 0; o < 27u; o++) {
                const int nx = (int)(bx >> 3) + (int)(o % 3u) - 1, ny = (int)(by >> 3) + (int)((o / 3u) % 3u) - 1, nz = (int)(bz >> 3) + (int)(o / 9u) - 1;
                if (((tiles >> o) & 1u) != 0u && nx >= 0 && nx < (int)J.nt[0] && ny >= 0 && ny < (int)J.nt[1] && nz >= 0 && nz < (int)J.nt[2])
                    act0[flood_tile_index((uint32_t)nx, (uint32_t)ny, (uint32_t)nz, J.nt)] = 1u;
            }
        }
    }
}

// one wave per tile: blockIdx.x is the tile index
template <int CONN>
__global__ __launch_bounds__(64) void k_flood_round(const FloodJob J, uint32_t* __restrict__ act_cur, uint32_t* __restrict__ act_next,
                                                     const uint32_t* __restrict__ prev, uint32_t* __restrict__ marked)
{
    __shared__ uint32_t ext[VRT_FLOOD_EXT_ROWS];
    __shared__ uint32_t s_wake;
    if (prev && *prev == 0u) return;                              // the round before marked nothing: the flood is done
    const uint32_t ti = blockIdx.x, lane = threadIdx.x;
    if (act_cur[ti] == 0u) return;                                // (wave-uniform)
    const uint32_t tx = ti % J.nt[0], ty = (ti / J.nt[0]) % J.nt[1], tz = ti / (J.nt[0] * J.nt[1]);
    if (lane == 0u) { act_cur[ti] = 0u; s_wake = 0u; }           // this buffer is the next round's target of nobody: only this wave touches the flag
    for (uint32_t e = lane; e < VRT_FLOOD_EXT_ROWS; e += 64u) ext[e] = flood_ext_row(CONN, J.reached, J.nt, tx, ty, tz, e);
    const uint32_t y = lane & 7u, z = lane >> 3, centre = (y + 1u) + 10u * (z + 1u);
    const uint32_t passable = J.passable[(size_t)ti * VRT_FLOOD_TILE_BYTES + lane];
    __syncthreads();
    const uint32_t before = (ext[centre] >> 1) & 0xFFu;
    uint32_t row = ext[centre];
    for (;;) {
        const uint32_t nw = flood_row_relax(CONN, ext, y, z, passable);
        if (__ballot(nw != row) == 0ull) break;                   // the wave's vote: no row changed
        __syncthreads();
        ext[centre] = row = nw;
        __syncthreads();
    }
    const uint32_t after = (row >> 1) & 0xFFu;
    if (after != before) J.reached[(size_t)ti * VRT_FLOOD_TILE_BYTES + lane] = (uint8_t)after;
    const uint32_t wake = flood_wake_mask(CONN, before, after, y, z);
    if (wake != 0u) atomicOr(&s_wake, wake);
    __syncthreads();
    if (lane < 27u && ((s_wake >> lane) & 1u) != 0u) {           // lane = (dx + 1) + 3 * (dy + 1) + 9 * (dz + 1)
        const int nx = (int)tx + (int)(lane % 3u) - 1, ny = (int)ty + (int)((lane / 3u) % 3u) - 1, nz = (int)tz + (int)(lane / 9u) - 1;
        if (nx >= 0 && nx < (int)J.nt[0] && ny >= 0 && ny < (int)J.nt[1] && nz >= 0 && nz < (int)J.nt[2]) {
            act_next[flood_tile_index((uint32_t)nx, (uint32_t)ny, (uint32_t)nz, J.nt)] = 1u;
            *marked = 1u;
        }
    }
}

// this lane's reached bit; (bx, by, bz) is an offset in J.box, which lies inside the clipped bounds
__device__ __forceinline__ bool flood_reached(const FloodJob& J, uint32_t bx, uint32_t by, uint32_t bz)
{
    const uint32_t rx = (uint32_t)(J.box.lo[0] - J.clo[0]) + bx, ry = (uint32_t)(J.box.lo[1] - J.clo[1]) + by, rz = (uint32_t)(J.box.lo[2] - J.clo[2]) + bz;
    return ((J.reached[flood_mask_byte(rx, ry, rz, J.nt)] >> flood_mask_bit(rx)) & 1u) != 0u;
}

// four waves per block, a segment each; J.box is the clipped bounds
__global__ __launch_bounds__(256) void k_flood_extent(const FloodJob J, FloodRecord* __restrict__ rec)
{
    __shared__ uint32_t s_region, s_count;
    __shared__ int32_t s_rmn[3], s_rmx[3], s_mn[3], s_mx[3];
    if (threadIdx.x < 3u) { s_rmn[threadIdx.x] = INT32_MAX; s_rmx[threadIdx.x] = INT32_MIN; s_mn[threadIdx.x] = INT32_MAX; s_mx[threadIdx.x] = INT32_MIN; }
    if (threadIdx.x == 0u) { s_region = 0u; s_count = 0u; }
    __syncthreads();
    const ReadBox& B = J.box;
    const uint32_t lane = threadIdx.x & 63u, g = blockIdx.x * 4u + (threadIdx.x >> 6);
    uint32_t seg, bx, by, bz;
    bool in_row;
    if (flood_lane(B, g, lane, seg, bx, by, bz, in_row)) {
        const bool inside = in_row && flood_reached(J, bx, by, bz);
        const uint64_t rmask = __ballot(inside);
        if (rmask != 0ull) {
            const int x = B.lo[0] + (int)bx, y = B.lo[1] + (int)by, z = B.lo[2] + (int)bz;
            const bool changed = inside && flood_read_voxel(B, x, y, z) != J.id;
            const uint64_t cmask = __ballot(changed);
            if (lane == 0u) {
                atomicAdd(&s_region, (uint32_t)__popcll(rmask));
                atomicMin(&s_rmn[0], x + (int)__builtin_ctzll(rmask)); atomicMax(&s_rmx[0], x + 63 - (int)__builtin_clzll(rmask));
                atomicMin(&s_rmn[1], y); atomicMax(&s_rmx[1], y);
                atomicMin(&s_rmn[2], z); atomicMax(&s_rmx[2], z);
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
    if (s_region == 0u) return;
    if (threadIdx.x == 0u) atomicAdd(&rec->region, (unsigned long long)s_region);
    if (threadIdx.x < 3u) { atomicMin(&rec->mn[threadIdx.x], s_rmn[threadIdx.x]); atomicMax(&rec->mx[threadIdx.x], s_rmx[threadIdx.x]); }
    if (s_count == 0u) return;
    if (threadIdx.x == 0u) { atomicAdd(&rec->edit.changed, (unsigned long long)s_count); atomicOr(&rec->edit.ids[J.id >> 5], 1u << (J.id & 31u)); }
    if (threadIdx.x < 3u) { atomicMin(&rec->edit.mn[threadIdx.x], s_mn[threadIdx.x]); atomicMax(&rec->edit.mx[threadIdx.x], s_mx[threadIdx.x]); }
}

// J.box is the tight box of the changed voxels
__global__ __launch_bounds__(256) void k_flood_compose(const FloodJob J, uint8_t* __restrict__ ids)
{
    const ReadBox& B = J.box;
    const uint32_t lane = threadIdx.x & 63u, g = blockIdx.x * 4u + (threadIdx.x >> 6);
    uint32_t seg, bx, by, bz;
    bool in_row;
    if (!flood_lane(B, g, lane, seg, bx, by, bz, in_row) || !in_row) return;
    const uint32_t nw = flood_reached(J, bx, by, bz) ? J.id : flood_read_voxel(B, B.lo[0] + (int)bx, B.lo[1] + (int)by, B.lo[2] + (int)bz);
    ids[read_box_index(bx, by, bz, B.size)] = (uint8_t)nw;
}

static uint32_t flood_blocks(const FloodJob& j)
{
    return (list_segments_per_row(j.box.size[0]) * j.box.size[1] * j.box.size[2] + 3u) / 4u;
}

hipError_t launch_flood_pass(const FloodJob& j, uint32_t* act0, FloodRecord* rec, hipStream_t s)
{
    hipLaunchKernelGGL(k_flood_pass, dim3(flood_blocks(j)), dim3(256), 0, s, j, act0, rec);
    return hipGetLastError();
}

hipError_t launch_flood_round(const FloodJob& j, uint32_t* act_cur, uint32_t* act_next, const uint32_t* prev, uint32_t* marked, hipStream_t s)
{
    const dim3 grid((uint32_t)flood_tile_count(j.nt)), block(64);
    switch (j.connectivity) {
    case VRT_FLOOD_CONN_FACES:   hipLaunchKernelGGL(k_flood_round<VRT_FLOOD_CONN_FACES>, grid, block, 0, s, j, act_cur, act_next, prev, marked); break;
    case VRT_FLOOD_CONN_CORNERS: hipLaunchKernelGGL(k_flood_round<VRT_FLOOD_CONN_CORNERS>, grid, block, 0, s, j, act_cur, act_next, prev, marked); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_flood_extent(const FloodJob& j, FloodRecord* rec, hipStream_t s)
{
    hipLaunchKernelGGL(k_flood_extent, dim3(flood_blocks(j)), dim3(256), 0, s, j, rec);
    return hipGetLastError();
}

hipError_t launch_flood_compose(const FloodJob& j, uint8_t* ids, hipStream_t s)
{
    hipLaunchKernelGGL(k_flood_compose, dim3(flood_blocks(j)), dim3(256), 0, s, j, ids);
    return hipGetLastError();
}

} // namespace vrt
