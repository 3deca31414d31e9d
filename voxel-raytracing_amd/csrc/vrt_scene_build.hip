// vrt_scene_build.hip -- scene build kernels for gfx950: occupancy pyramid, clearance fields, open cells, bricks, padding.
#include "vrt_device_common.h"

namespace vrt {

// ---------------------------------------------------------------------------------------------
// occupancy pyramid build
// ---------------------------------------------------------------------------------------------

__global__ void k_build_occ1(const uint8_t* __restrict__ vox, int W, int H, int D,
                             uint64_t* __restrict__ occ1, int n1x, int n1y, int n1z)
{
    int cx = blockIdx.x * blockDim.x + threadIdx.x;
    int cy = blockIdx.y, cz = blockIdx.z;
    if (cx >= n1x) return;
    uint64_t w = 0;
    for (int z = 0; z < 4; z++) {
        int vz = cz * 4 + z;
        if (vz >= D) break;
        for (int y = 0; y < 4; y++) {
            int vy = cy * 4 + y;
            if (vy >= H) break;
            size_t base = (size_t)cx * 4 + ((size_t)vy + (size_t)vz * H) * W;
            for (int x = 0; x < 4; x++) {
                int vx = cx * 4 + x;
                if (vx < W && vox[base + x] != 0) w |= 1ull << (x | (y << 2) | (z << 4));
            }
        }
    }
    occ1[(size_t)cx + ((size_t)cy + (size_t)cz * n1y) * n1x] = w;
}

// level k+1 from level k: bit set <=> child word != 0
__global__ void k_build_occ_up(const uint64_t* __restrict__ lo, int lx, int ly, int lz,
                               uint64_t* __restrict__ hi, int hx, int hy, int hz)
{
    int cx = blockIdx.x * blockDim.x + threadIdx.x;
    int cy = blockIdx.y, cz = blockIdx.z;
    if (cx >= hx) return;
    uint64_t w = 0;
    for (int z = 0; z < 4; z++) {
        int vz = cz * 4 + z;
        if (vz >= lz) break;
        for (int y = 0; y < 4; y++) {
            int vy = cy * 4 + y;
            if (vy >= ly) break;
            for (int x = 0; x < 4; x++) {
                int vx = cx * 4 + x;
                if (vx < lx && lo[(size_t)vx + ((size_t)vy + (size_t)vz * ly) * lx] != 0)
                    w |= 1ull << (x | (y << 2) | (z << 4));
            }
        }
    }
    hi[(size_t)cx + ((size_t)cy + (size_t)cz * hy) * hx] = w;
}

hipError_t launch_build_pyramid(const uint8_t* vox, int W, int H, int D, uint64_t* occ1, uint64_t* occ2,
                                uint64_t* occ3, hipStream_t s)
{
    int n1x = (W + 3) / 4, n1y = (H + 3) / 4, n1z = (D + 3) / 4;
    int n2x = (n1x + 3) / 4, n2y = (n1y + 3) / 4, n2z = (n1z + 3) / 4;
    int n3x = (n2x + 3) / 4, n3y = (n2y + 3) / 4, n3z = (n2z + 3) / 4;
    hipLaunchKernelGGL(k_build_occ1, dim3((n1x + 63) / 64, n1y, n1z), dim3(64), 0, s, vox, W, H, D, occ1, n1x, n1y, n1z);
    hipLaunchKernelGGL(k_build_occ_up, dim3((n2x + 63) / 64, n2y, n2z), dim3(64), 0, s, occ1, n1x, n1y, n1z, occ2, n2x, n2y, n2z);
    hipLaunchKernelGGL(k_build_occ_up, dim3((n3x + 63) / 64, n3y, n3z), dim3(64), 0, s, occ2, n2x, n2y, n2z, occ3, n3x, n3y, n3z);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// clearance fields (scene build).  For octant o = (sx, sy, sz) in {-1,+1}^3, c_o(p) = side of the largest empty
// cube with corner p extending towards (sx, sy, sz), 0 for a solid voxel, capped at `cap` (VRT_DF_CAP = 127 for
// the voxel fields, 16 for the bricks' coarse fields):
//   c(p) = min_{c>=0} max(c, min_{b>=0} max(b, min_{a>=0} max(a, solid(p + (a sx, b sy, c sz)) ? 0 : INF)))
// i.e. three one-sided 1-D min-max passes.  Outside the volume counts as solid, so a run never carries a ray more
// than one voxel past a wall.
// ---------------------------------------------------------------------------------------------

// src == nullptr: first pass, the field is (vox != 0 ? 0 : INF).
__global__ __launch_bounds__(256) void k_df_pass(const uint8_t* __restrict__ vox, const uint8_t* __restrict__ src,
                                                 uint8_t* __restrict__ dst, int W, int H, int D, int axis, int dir, int padded, int cap)
{
    size_t n = (size_t)W * H * D;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int x = (int)(i % (size_t)W), y = (int)((i / (size_t)W) % (size_t)H), z = (int)(i / ((size_t)W * H));
    int pos = axis == 0 ? x : (axis == 1 ? y : z);
    int dim = axis == 0 ? W : (axis == 1 ? H : D);
    long long stride = (axis == 0 ? 1 : (axis == 1 ? (long long)W : (long long)W * H)) * dir;
    int best = src ? (int)src[i] : (vox[i] != 0 ? 0 : cap + 1);
    for (int t = 1; t < best; t++) {
        int q = pos + t * dir;
        int val = (q < 0 || q >= dim) ? 0
                                      : (src ? (int)src[(long long)i + t * stride] : (vox[(long long)i + t * stride] != 0 ? 0 : cap + 1));
        int m = val > t ? val : t;
        best = best < m ? best : m;
    }
    size_t o = i;
    if (padded) {                                            // final pass: into the zero-bordered field (vrt_volume.h df_index)
        o = (size_t)(x + 1) + ((size_t)(y + 1) + (size_t)(z + 1) * ((size_t)H + 2u)) * ((size_t)W + 2u);
    }
    dst[o] = (uint8_t)(best > cap ? cap : best);
}

// df: 8 * stride bytes (stride = df_field_bytes: one zero-bordered field); tmp0/tmp1: W*H*D bytes each
hipError_t launch_build_df(const uint8_t* vox, int W, int H, int D, uint8_t* df, size_t stride, uint8_t* tmp0, uint8_t* tmp1, hipStream_t s, int cap)
{
    if (cap <= 0) cap = VRT_DF_CAP;
    size_t n = (size_t)W * H * D;
    unsigned blocks = (unsigned)((n + 255) / 256);
    for (int o = 0; o < 8; o++) {
        int sx = (o & 1) ? 1 : -1, sy = (o & 2) ? 1 : -1, sz = (o & 4) ? 1 : -1;
        hipLaunchKernelGGL(k_df_pass, dim3(blocks), dim3(256), 0, s, vox, (const uint8_t*)nullptr, tmp0, W, H, D, 0, sx, 0, cap);
        hipLaunchKernelGGL(k_df_pass, dim3(blocks), dim3(256), 0, s, vox, (const uint8_t*)tmp0, tmp1, W, H, D, 1, sy, 0, cap);
        hipLaunchKernelGGL(k_df_pass, dim3(blocks), dim3(256), 0, s, vox, (const uint8_t*)tmp1, df + (size_t)o * stride, W, H, D, 2, sz, 1, cap);
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// open cells.  A ray only ever moves towards the signs of its direction, so from voxel p it can only meet voxels of the box
// between p and the volume's corner in its octant.  Where that whole box is empty the ray is a miss, whatever it would still
// walk through: the octant's field holds 0 there -- the code of "the march ends here", as at a solid voxel and in the border;
// the voxel id read at the same index (0) then says miss.  Hits are untouched (a ray that hits never stands on such a cell);
// what a miss leaves behind does not depend on where it left the volume (traceRay, frag:176-196: material, position and
// normal of a miss are 0) -- only the NUMBER of iterations does, which the count planes report: those are rendered through a
// copy of the fields without open cells (vrt_api.hip).
//   open(p) = AND over a, b, c >= 0 of empty(p + (a sx, b sy, c sz)): three one-sided AND scans.
// ---------------------------------------------------------------------------------------------

// scan along y (axis 1; blockIdx.y = z) or z (axis 2; blockIdx.y = y): one thread per line, x across the threads
__global__ __launch_bounds__(256) void k_open_scan(const uint8_t* __restrict__ vox, const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                   int W, int H, int D, int axis, int dir)
{
    const int x = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (x >= W) return;
    const int len = axis == 1 ? H : D;
    const size_t step = axis == 1 ? (size_t)W : (size_t)W * (size_t)H;
    const size_t base = (size_t)x + (axis == 1 ? (size_t)blockIdx.y * (size_t)W * (size_t)H : (size_t)blockIdx.y * (size_t)W);
    uint8_t flag = 1;
    for (int t = 0; t < len; t++) {                            // from the far end of the line towards the near one
        const size_t i = base + (size_t)(dir > 0 ? len - 1 - t : t) * step;
        flag &= src ? src[i] : (uint8_t)(vox[i] == 0);
        dst[i] = flag;
    }
}

// scan along x, one wave per line, and the result: 0 into the octant's zero-bordered field where the cell is open
__global__ __launch_bounds__(256) void k_open_x(const uint8_t* __restrict__ src, uint8_t* __restrict__ field, int W, int H, int D, int dir, int mark)
{
    const int lane = (int)(threadIdx.x & 63u);
    const size_t line = (size_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (line >= (size_t)H * (size_t)D) return;                 // wave-uniform
    const int y = (int)(line % (size_t)H), z = (int)(line / (size_t)H);
    const uint8_t* row = src + line * (size_t)W;
    uint8_t* out = field + 1 + ((size_t)(y + 1) + (size_t)(z + 1) * ((size_t)H + 2u)) * ((size_t)W + 2u);
    bool carry = true;
    const int chunks = (W + 63) / 64;
    for (int c = 0; c < chunks; c++) {
        const int x = (dir > 0 ? chunks - 1 - c : c) * 64 + lane;
        const bool f = x < W ? row[x] != 0 : true;
        const uint64_t blocked = ~__ballot(f);
        const bool open = carry && f && (dir > 0 ? (blocked >> lane) == 0ull : (blocked << (63 - lane)) == 0ull);
        if (x < W && open) out[x] = mark ? (uint8_t)(out[x] | (uint8_t)mark) : (uint8_t)0;   // bricks: bit 7; voxels: the code 0
        carry = carry && blocked == 0ull;
    }
}

hipError_t launch_open_cells(const uint8_t* vox, int W, int H, int D, uint8_t* df, size_t stride, uint8_t* tmp0, uint8_t* tmp1, hipStream_t s, int mark)
{
    const unsigned bx = (unsigned)((W + 255) / 256);
    const size_t lines = (size_t)H * (size_t)D;
    for (int o = 0; o < 8; o++) {
        const int sx = (o & 1) ? 1 : -1, sy = (o & 2) ? 1 : -1, sz = (o & 4) ? 1 : -1;
        hipLaunchKernelGGL(k_open_scan, dim3(bx, (unsigned)D), dim3(256), 0, s, vox, (const uint8_t*)nullptr, tmp0, W, H, D, 1, sy);
        hipLaunchKernelGGL(k_open_scan, dim3(bx, (unsigned)H), dim3(256), 0, s, vox, (const uint8_t*)tmp0, tmp1, W, H, D, 2, sz);
        hipLaunchKernelGGL(k_open_x, dim3((unsigned)((lines + 3) / 4)), dim3(256), 0, s, (const uint8_t*)tmp1, df + (size_t)o * stride, W, H, D, sx, mark);
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// brick scenes (vrt_scene_from_bricks): padded pointer grid, brick occupancy, per-voxel clearance of the occupied bricks
// ---------------------------------------------------------------------------------------------

// grid (nbx * nby * nbz) -> interior of the padded grid ((nbx+2)(nby+2)(nbz+2); its border was preset to 0xFFFFFFFF = outside
// the volume) and one byte per brick: occupied or not
__global__ __launch_bounds__(256) void k_brick_grid(const uint32_t* __restrict__ grid, int nbx, int nby, int nbz,
                                                    uint32_t* __restrict__ padded, uint8_t* __restrict__ occ)
{
    const size_t n = (size_t)nbx * nby * nbz, i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int x = (int)(i % (size_t)nbx), y = (int)((i / (size_t)nbx) % (size_t)nby), z = (int)(i / ((size_t)nbx * nby));
    const uint32_t g = grid[i];
    padded[(size_t)(x + 1) + ((size_t)(y + 1) + (size_t)(z + 1) * ((size_t)nby + 2u)) * ((size_t)nbx + 2u)] = g;
    occ[i] = g != 0u ? 1 : 0;
}

// One workgroup per occupied brick: the clearance of each of its voxels in each octant, looking through the 26 neighbours
// (24^3 voxels in LDS; beyond them -- and outside the volume -- counts as solid, so values reach 9..16).  Per octant the
// three one-sided min-max passes of k_df_pass, restricted to the cells the centre brick's results depend on.
#define VRT_FINE_CAP 16
// b: the brick's pool index; pc: its index in the padded grid
__device__ __forceinline__ void brick_fine_body(const uint32_t* __restrict__ padded, int pbx, int pby, const uint32_t b, const uint32_t pc,
                                                const uint8_t* __restrict__ pool, uint8_t* __restrict__ fine)
{
    __shared__ uint8_t A[24 * 24 * 24], B[24 * 24 * 24];
    const int cbx = (int)(pc % (uint32_t)pbx), cby = (int)((pc / (uint32_t)pbx) % (uint32_t)pby), cbz = (int)(pc / ((uint32_t)pbx * (uint32_t)pby));
    __shared__ uint32_t nb[27];                               // the 3 x 3 x 3 bricks around it: 0 empty, 0xFFFFFFFF outside the volume
    if (threadIdx.x < 27) {
        const int dx = (int)threadIdx.x % 3 - 1, dy = ((int)threadIdx.x / 3) % 3 - 1, dz = (int)threadIdx.x / 9 - 1;
        nb[threadIdx.x] = padded[(size_t)(cbx + dx) + ((size_t)(cby + dy) + (size_t)(cbz + dz) * (size_t)pby) * (size_t)pbx];
    }
    __syncthreads();
    for (int t = threadIdx.x; t < 24 * 24 * 24; t += 256) {
        const int x = t % 24, y = (t / 24) % 24, z = t / 576;
        const int k = (x >> 3) + (y >> 3) * 3 + (z >> 3) * 9;
        const uint32_t ptr = nb[k];
        uint8_t solid;
        if (ptr == 0xFFFFFFFFu) solid = 1;                     // outside the volume
        else if (ptr == 0u) solid = 0;
        else solid = pool[(size_t)(ptr - 1u) * 512u + (size_t)((x & 7) + (y & 7) * 8 + (z & 7) * 64)] != 0 ? 1 : 0;
        A[t] = solid ? 0 : VRT_FINE_CAP + 1;
    }
    __syncthreads();
    for (int o = 0; o < 8; o++) {
        const int sx = (o & 1) ? 1 : -1, sy = (o & 2) ? 1 : -1, sz = (o & 4) ? 1 : -1;
        // pass x: centre columns, every y and z     A -> B
        for (int t = threadIdx.x; t < 8 * 24 * 24; t += 256) {
            const int x = 8 + (t & 7), y = (t >> 3) % 24, z = (t >> 3) / 24;
            const int i = x + y * 24 + z * 576;
            int best = A[i];
            for (int k = 1; k < best; k++) {
                const int q = x + k * sx;
                const int val = (q < 0 || q >= 24) ? 0 : (int)A[i + k * sx];
                const int m = val > k ? val : k;
                best = best < m ? best : m;
            }
            B[i] = (uint8_t)best;
        }
        __syncthreads();
        // pass y: centre columns and rows, every z; the results go to the x-columns 0..7 of B, which this pass does not read
        for (int t = threadIdx.x; t < 8 * 8 * 24; t += 256) {
            const int x = 8 + (t & 7), y = 8 + ((t >> 3) & 7), z = t >> 6;
            const int i = x + y * 24 + z * 576;
            int best = B[i];
            for (int k = 1; k < best; k++) {
                const int q = y + k * sy;
                const int val = (q < 0 || q >= 24) ? 0 : (int)B[i + k * sy * 24];
                const int m = val > k ? val : k;
                best = best < m ? best : m;
            }
            B[(x - 8) + y * 24 + z * 576] = (uint8_t)best;
        }
        __syncthreads();
        // pass z: the centre brick
        for (int t = threadIdx.x; t < 512; t += 256) {
            const int lx = t & 7, ly = (t >> 3) & 7, lz = t >> 6;
            const int z = 8 + lz;
            const int i = lx + (8 + ly) * 24 + z * 576;
            int best = B[i];
            for (int k = 1; k < best; k++) {
                const int q = z + k * sz;
                const int val = (q < 0 || q >= 24) ? 0 : (int)B[i + k * sz * 576];
                const int m = val > k ? val : k;
                best = best < m ? best : m;
            }
            fine[((size_t)b * 8u + (size_t)o) * 512u + (size_t)t] = (uint8_t)(best > VRT_FINE_CAP ? VRT_FINE_CAP : best);
        }
        __syncthreads();
    }
}

// the build: every pool brick, its padded index from coord[]
__global__ __launch_bounds__(256) void k_brick_fine(const uint32_t* __restrict__ padded, int pbx, int pby, const uint32_t* __restrict__ coord,
                                                    const uint8_t* __restrict__ pool, uint8_t* __restrict__ fine)
{
    brick_fine_body(padded, pbx, pby, blockIdx.x, coord[blockIdx.x], pool, fine);
}

// scene edits: the listed bricks, list[i] = (pool index, padded index)
__global__ __launch_bounds__(256) void k_brick_fine_list(const uint32_t* __restrict__ padded, int pbx, int pby, const uint2* __restrict__ list,
                                                         const uint8_t* __restrict__ pool, uint8_t* __restrict__ fine)
{
    const uint2 e = list[blockIdx.x];
    brick_fine_body(padded, pbx, pby, e.x, e.y, pool, fine);
}

// vrt_scene_reserve_bricks: the padded pointer grid and the occupancy bytes back out of the packed entries
__global__ __launch_bounds__(256) void k_brick_unpack(const uint64_t* __restrict__ entry, int nbx, int nby, int nbz,
                                                      uint32_t* __restrict__ padded, uint8_t* __restrict__ occ)
{
    const size_t pbx = (size_t)nbx + 2u, pby = (size_t)nby + 2u, npad = pbx * pby * ((size_t)nbz + 2u);
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npad) return;
    const int x = (int)(i % pbx) - 1, y = (int)((i / pbx) % pby) - 1, z = (int)(i / (pbx * pby)) - 1;
    const uint32_t ptr = (uint32_t)entry[i] & 0xFFFFFFu;
    if (x < 0 || y < 0 || z < 0 || x >= nbx || y >= nby || z >= nbz) { padded[i] = 0xFFFFFFFFu; return; }
    padded[i] = ptr;
    occ[(size_t)x + ((size_t)y + (size_t)z * (size_t)nby) * (size_t)nbx] = ptr != 0u ? 1 : 0;
}

// the padded pointer grid and the eight coarse fields folded into the one word per brick the march reads (brick_entry_pack)
__global__ __launch_bounds__(256) void k_brick_pack(const uint32_t* __restrict__ padded, const uint8_t* __restrict__ coarse, size_t cstride,
                                                    size_t npad, uint64_t* __restrict__ entry)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npad) return;
    uint8_t c8[8];
#pragma unroll
    for (int o = 0; o < 8; o++) c8[o] = coarse[(size_t)o * cstride + i];
    entry[i] = brick_entry_pack(padded[i], c8);
}

hipError_t launch_brick_pack(const uint32_t* padded, const uint8_t* coarse, size_t cstride, size_t npad, uint64_t* entry, hipStream_t s)
{
    hipLaunchKernelGGL(k_brick_pack, dim3((unsigned)((npad + 255) / 256)), dim3(256), 0, s, padded, coarse, cstride, npad, entry);
    return hipGetLastError();
}

hipError_t launch_brick_grid(const uint32_t* grid, int nbx, int nby, int nbz, uint32_t* padded, uint8_t* occ, hipStream_t s)
{
    const size_t n = (size_t)nbx * nby * nbz;
    hipLaunchKernelGGL(k_brick_grid, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, grid, nbx, nby, nbz, padded, occ);
    return hipGetLastError();
}

hipError_t launch_brick_fine(const uint32_t* padded, int pbx, int pby, const uint32_t* coord, uint32_t n_bricks, const uint8_t* pool,
                             uint8_t* fine, hipStream_t s)
{
    if (n_bricks == 0) return hipSuccess;
    hipLaunchKernelGGL(k_brick_fine, dim3(n_bricks), dim3(256), 0, s, padded, pbx, pby, coord, pool, fine);
    return hipGetLastError();
}

hipError_t launch_brick_fine_list(const uint32_t* padded, int pbx, int pby, const uint2* list, uint32_t n_list, const uint8_t* pool,
                                  uint8_t* fine, hipStream_t s)
{
    if (n_list == 0) return hipSuccess;
    hipLaunchKernelGGL(k_brick_fine_list, dim3(n_list), dim3(256), 0, s, padded, pbx, pby, list, pool, fine);
    return hipGetLastError();
}

hipError_t launch_brick_unpack(const uint64_t* entry, int nbx, int nby, int nbz, uint32_t* padded, uint8_t* occ, hipStream_t s)
{
    const size_t npad = ((size_t)nbx + 2u) * ((size_t)nby + 2u) * ((size_t)nbz + 2u);
    hipLaunchKernelGGL(k_brick_unpack, dim3((unsigned)((npad + 255) / 256)), dim3(256), 0, s, entry, nbx, nby, nbz, padded, occ);
    return hipGetLastError();
}

// field 8 of the clearance allocation: the voxel ids in the fields' zero-bordered layout (trace_df_fast reads the id of a hit
// at the index it already has); the border stays 0
__global__ __launch_bounds__(256) void k_pad_vox(const uint8_t* __restrict__ vox, uint8_t* __restrict__ dst, int W, int H, int D)
{
    size_t n = (size_t)W * H * D;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int x = (int)(i % (size_t)W), y = (int)((i / (size_t)W) % (size_t)H), z = (int)(i / ((size_t)W * H));
    dst[(size_t)(x + 1) + ((size_t)(y + 1) + (size_t)(z + 1) * ((size_t)H + 2u)) * ((size_t)W + 2u)] = vox[i];
}

hipError_t launch_pad_vox(const uint8_t* vox, int W, int H, int D, uint8_t* dst, hipStream_t s)
{
    size_t n = (size_t)W * H * D;
    hipLaunchKernelGGL(k_pad_vox, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, vox, dst, W, H, D);
    return hipGetLastError();
}

} // namespace vrt
