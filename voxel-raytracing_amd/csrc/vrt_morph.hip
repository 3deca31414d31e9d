// vrt_morph.hip -- binary morphology for gfx950 (vrt_scene_morph): grow, shrink, open, close or hollow the scene's solid on the
// device, then hand what changes to the edits as a brush hands over its shape.  vrt_morph.h has the definition, the masks'
// layout and the argument that a tile with a halo of r is exact after r steps, vrt_morph_launch.h the job.
//   k_morph_pass         k_flood_pass's scheme over the DOMAIN (the clipped bounds grown by the halo): one wave per segment of 64
//                        cells of a row, a lane reads its cell -- the border's value beyond the volume -- the wave ballots
//                        id != 0; the ballot's two row words are stored by two lanes.
//   k_morph_step<CONN>   one workgroup of 256 per tile of 2 row words x 16 x 16 rows: the extended block (one more word either
//                        side in x, r more rows either side in y and z) into LDS, r unit steps there between two buffers
//                        (morph_ext_step, the rows a later step still reads: morph_ext_live), the tile's rows out.  An erosion
//                        complements the words on the way in and on the way out.  32-bit row words, consecutive lanes on
//                        consecutive words: no bank conflict on the centre reads.
//   k_morph_extent       k_brush_extent with "inside" replaced by (in R, was solid): counts, bounds, the id when a voxel is added,
//                        plus `added` and `removed`.
//   k_morph_compose      k_brush_compose likewise: the tight box's new ids into the edits' scratch in read_box_index order.
// A dense scene and a brick scene share the kernels (a wave-uniform branch on the view): an absent brick costs the 32-bit load of
// the low half of its entry and reads no pool.  No wave waits for another; ordinary vector loads and stores, wave votes, LDS; no
// inline assembly.
#include "vrt_device_common.h"
#include "vrt_morph_launch.h"

namespace vrt {

__device__ __forceinline__ uint32_t morph_read_voxel(const ReadBox& B, int x, int y, int z)
{
    if (B.vox) return B.vox[(size_t)x + ((size_t)y + (size_t)z * (size_t)B.H) * (size_t)B.W];
    const size_t pc = (size_t)((x >> 3) + 1) + ((size_t)((y >> 3) + 1) + (size_t)((z >> 3) + 1) * (size_t)B.pby) * (size_t)B.pbx;
    const uint32_t ptr = ((const uint32_t*)B.bentry)[2u * pc] & 0xFFFFFFu;          // the entry's low word: pointer | open bits << 24
    if (ptr == 0u || ptr > B.bcap) return 0u;
    return B.bpool[(size_t)(ptr - 1u) * 512u + (size_t)((x & 7) | ((y & 7) << 3) | ((z & 7) << 6))];
}

// segment g of a box of the sides `size` -> this lane's offset in it; in_row: the lane lies in the row.  false: no such segment
// (wave-uniform)
__device__ __forceinline__ bool morph_lane(const uint32_t size[3], uint32_t g, uint32_t lane, uint32_t& seg, uint32_t& bx, uint32_t& by, uint32_t& bz, bool& in_row)
{
    const uint32_t spr = list_segments_per_row(size[0]);
    if (g >= spr * size[1] * size[2]) return false;
    const uint32_t row = g / spr;
    seg = g - row * spr;
    bx = seg * VRT_LIST_SEGMENT + lane;
    bz = row / size[1];
    by = row - bz * size[1];
    in_row = bx < size[0];
    return true;
}

// four waves per block, a segment of the domain each
__global__ __launch_bounds__(256) void k_morph_pass(const MorphJob J)
{
    const uint32_t lane = threadIdx.x & 63u, g = blockIdx.x * 4u + (threadIdx.x >> 6);
    uint32_t seg, mx, my, mz;
    bool in_row;
    if (!morph_lane(J.msize, g, lane, seg, mx, my, mz, in_row)) return;
    const int x = J.mlo[0] + (int)mx, y = J.mlo[1] + (int)my, z = J.mlo[2] + (int)mz;
    bool solid = false;
    if (in_row) {
        if (x < 0 || x >= J.dim[0] || y < 0 || y >= J.dim[1] || z < 0 || z >= J.dim[2]) solid = J.border_solid != 0u;
        else solid = morph_read_voxel(J.box, x, y, z) != 0u;
    }
    const uint64_t mask = __ballot(solid);
    const uint32_t wx = seg * 2u + lane;                          // lanes 0 and 1: the segment's two row words
    if (lane < 2u && wx < morph_row_words(J.msize[0])) J.mask[0][morph_word_index(wx, my, mz, J.msize)] = (uint32_t)(mask >> (32u * lane));
}

// one workgroup per tile: blockIdx is the tile
template <int CONN>
__global__ __launch_bounds__(256) void k_morph_step(const MorphJob J, const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, const uint32_t erode)
{
    __shared__ uint32_t ext[2][VRT_MORPH_EXT_MAX];
    const uint32_t r = J.radius, E = morph_ext_rows(r), n = morph_ext_count(r);
    const uint32_t tx = blockIdx.x, ty = blockIdx.y, tz = blockIdx.z;
    for (uint32_t i = threadIdx.x; i < n; i += 256u) ext[0][i] = morph_ext_load(src, J.msize, erode != 0u, tx, ty, tz, r, i);
    __syncthreads();
    uint32_t cur = 0u;
    for (uint32_t k = 1u; k <= r; k++) {                          // (r is the launch's: every wave makes the same trips)
        for (uint32_t i = threadIdx.x; i < n; i += 256u) {
            const uint32_t xw = i % VRT_MORPH_EXT_WORDS, row = i / VRT_MORPH_EXT_WORDS, ey = row % E, ez = row / E;
            if (morph_ext_live(E, k, ey, ez)) ext[cur ^ 1u][i] = morph_ext_step(CONN, ext[cur], E, xw, ey, ez);
        }
        __syncthreads();
        cur ^= 1u;
    }
    // the tile's own words: 2 x 16 x 16, two per thread
    const uint32_t nw = morph_row_words(J.msize[0]);
    for (uint32_t i = threadIdx.x; i < VRT_MORPH_TILE_WORDS * VRT_MORPH_TILE_ROWS * VRT_MORPH_TILE_ROWS; i += 256u) {
        const uint32_t xw = i % VRT_MORPH_TILE_WORDS, ty_ = (i / VRT_MORPH_TILE_WORDS) % VRT_MORPH_TILE_ROWS, tz_ = i / (VRT_MORPH_TILE_WORDS * VRT_MORPH_TILE_ROWS);
        const uint32_t gw = tx * VRT_MORPH_TILE_WORDS + xw, gy = ty * VRT_MORPH_TILE_ROWS + ty_, gz = tz * VRT_MORPH_TILE_ROWS + tz_;
        if (gw >= nw || gy >= J.msize[1] || gz >= J.msize[2]) continue;
        const uint32_t v = ext[cur][morph_ext_index(xw + 1u, ty_ + r, tz_ + r, E)];
        dst[morph_word_index(gw, gy, gz, J.msize)] = erode != 0u ? ~v : v;
    }
}

// segment g of J.box -> this lane's voxel, its id and what it becomes; false: no such segment (wave-uniform)
__device__ __forceinline__ bool morph_voxel(const MorphJob& J, uint32_t g, uint32_t lane, uint32_t& bx, uint32_t& by, uint32_t& bz, bool& in_row, uint32_t& old, uint32_t& nw)
{
    const ReadBox& B = J.box;
    uint32_t seg;
    if (!morph_lane(B.size, g, lane, seg, bx, by, bz, in_row)) return false;
    old = 0u; nw = 0u;
    if (in_row) {
        const int x = B.lo[0] + (int)bx, y = B.lo[1] + (int)by, z = B.lo[2] + (int)bz;       // inside the clipped bounds: inside the volume and the domain
        old = morph_read_voxel(B, x, y, z);
        nw = morph_value(J.op, morph_mask_bit(J.result, (uint32_t)(x - J.mlo[0]), (uint32_t)(y - J.mlo[1]), (uint32_t)(z - J.mlo[2]), J.msize), old, J.id);
    }
    return true;
}

// four waves per block, a segment each; J.box is the clipped bounds
__global__ __launch_bounds__(256) void k_morph_extent(const MorphJob J, MorphRecord* __restrict__ rec)
{
    __shared__ uint32_t s_count, s_added;
    __shared__ int32_t s_mn[3], s_mx[3];
    if (threadIdx.x < 3u) { s_mn[threadIdx.x] = INT32_MAX; s_mx[threadIdx.x] = INT32_MIN; }
    if (threadIdx.x == 0u) { s_count = 0u; s_added = 0u; }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, g = blockIdx.x * 4u + (threadIdx.x >> 6);
    uint32_t bx, by, bz, old, nw;
    bool in_row;
    if (morph_voxel(J, g, lane, bx, by, bz, in_row, old, nw)) {
        const bool changed = in_row && nw != old;
        const uint64_t mask = __ballot(changed);
        if (mask != 0ull) {
            const uint64_t amask = __ballot(changed && old == 0u);
            if (lane == 0u) {
                const int x0 = J.box.lo[0] + (int)(bx + (uint32_t)__builtin_ctzll(mask)), x1 = J.box.lo[0] + (int)(bx + 63u - (uint32_t)__builtin_clzll(mask));
                const int y = J.box.lo[1] + (int)by, z = J.box.lo[2] + (int)bz;
                atomicAdd(&s_count, (uint32_t)__popcll(mask));
                atomicAdd(&s_added, (uint32_t)__popcll(amask));
                atomicMin(&s_mn[0], x0); atomicMax(&s_mx[0], x1);
                atomicMin(&s_mn[1], y);  atomicMax(&s_mx[1], y);
                atomicMin(&s_mn[2], z);  atomicMax(&s_mx[2], z);
            }
        }
    }
    __syncthreads();
    if (s_count == 0u) return;
    if (threadIdx.x == 0u) {
        atomicAdd(&rec->edit.changed, (unsigned long long)s_count);
        if (s_added != 0u) { atomicAdd(&rec->added, (unsigned long long)s_added); atomicOr(&rec->edit.ids[J.id >> 5], 1u << (J.id & 31u)); }
        if (s_count != s_added) atomicAdd(&rec->removed, (unsigned long long)(s_count - s_added));
    }
    if (threadIdx.x < 3u) { atomicMin(&rec->edit.mn[threadIdx.x], s_mn[threadIdx.x]); atomicMax(&rec->edit.mx[threadIdx.x], s_mx[threadIdx.x]); }
}

// J.box is the tight box of the changed voxels
__global__ __launch_bounds__(256) void k_morph_compose(const MorphJob J, uint8_t* __restrict__ ids)
{
    const uint32_t lane = threadIdx.x & 63u, g = blockIdx.x * 4u + (threadIdx.x >> 6);
    uint32_t bx, by, bz, old, nw;
    bool in_row;
    if (!morph_voxel(J, g, lane, bx, by, bz, in_row, old, nw)) return;
    if (in_row) ids[read_box_index(bx, by, bz, J.box.size)] = (uint8_t)nw;
}

static uint32_t morph_blocks(const uint32_t size[3])
{
    return (list_segments_per_row(size[0]) * size[1] * size[2] + 3u) / 4u;
}

hipError_t launch_morph_pass(const MorphJob& j, hipStream_t s)
{
    hipLaunchKernelGGL(k_morph_pass, dim3(morph_blocks(j.msize)), dim3(256), 0, s, j);
    return hipGetLastError();
}

hipError_t launch_morph_step(const MorphJob& j, const uint32_t* src, uint32_t* dst, bool erode, hipStream_t s)
{
    uint32_t nt[3];
    morph_tiles(j.msize, nt);
    if (j.radius < 1u || j.radius > VRT_MORPH_MAX_RADIUS) return hipErrorInvalidValue;      // (the extended block is sized for it)
    const dim3 grid(nt[0], nt[1], nt[2]), block(256);
    switch (j.connectivity) {
    case VRT_MORPH_CONN_FACES:   hipLaunchKernelGGL(k_morph_step<VRT_MORPH_CONN_FACES>, grid, block, 0, s, j, src, dst, erode ? 1u : 0u); break;
    case VRT_MORPH_CONN_CORNERS: hipLaunchKernelGGL(k_morph_step<VRT_MORPH_CONN_CORNERS>, grid, block, 0, s, j, src, dst, erode ? 1u : 0u); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_morph_extent(const MorphJob& j, MorphRecord* rec, hipStream_t s)
{
    hipLaunchKernelGGL(k_morph_extent, dim3(morph_blocks(j.box.size)), dim3(256), 0, s, j, rec);
    return hipGetLastError();
}

hipError_t launch_morph_compose(const MorphJob& j, uint8_t* ids, hipStream_t s)
{
    hipLaunchKernelGGL(k_morph_compose, dim3(morph_blocks(j.box.size)), dim3(256), 0, s, j, ids);
    return hipGetLastError();
}

} // namespace vrt
