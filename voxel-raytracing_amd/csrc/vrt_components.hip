// vrt_components.hip -- connected-component labelling for gfx950 (vrt_scene_components, vrt_scene_component_labels,
// vrt_scene_filter_components): a concurrent union-find over the label volume, then numbering, measuring and the filter's
// edit.  vrt_components.h has the definition, the passes and the argument why the result does not depend on the schedule,
// vrt_components_launch.h the job.
//   k_comp_tile<CONN, SAME>  one wave (a block of 64) per tile, a lane per row (y, z) holding the row's 8 keys and labels in
//                            registers.  The labels also lie in LDS with a border of "no label" around the tile; a lane takes
//                            the minimum over its voxels' joined neighbours, then runs it along the row in registers both
//                            ways; a wave vote ends the loop.  Writes the label volume.
//   k_comp_seam<CONN>        a thread per voxel on a tile's boundary: for each forward direction whose neighbour lies in another
//                            tile and is joined, comp_unite.  Parents are read with relaxed loads of device scope, linked with
//                            atomicMin (device scope).  No wave waits for another.
//   k_comp_flatten           a wave per segment of 64 voxels of a row: every label becomes its root; a ballot counts the roots.
//   k_comp_number            the same segments: a root's number from the scanned counts and its rank in the ballot; it writes
//                            its table entry and VRT_COMP_NUMBERED | number in its own word.
//   k_comp_measure           a wave per tile, a lane per row: labels become VRT_COMP_NUMBERED | number; for each component in the
//                            tile, eight ballots give count and box in scalar registers, seven lanes issue one atomic each.
//   k_comp_summary           a thread per component: a wave's max of the largest-key and sum of the counts, one atomic each.
//   k_comp_select            a thread per component: the filter's verdict into the table; selected components and voxels summed.
//   k_comp_extent / _compose k_flood_extent / k_flood_compose with "inside" = the voxel's component is selected.
//   k_comp_labels            a box of the label volume without the NUMBERED bit, for the host.
// Ordinary vector loads, stores and atomics, wave votes, LDS; no inline assembly.
#include "vrt_device_common.h"
#include "vrt_components_launch.h"

namespace vrt {

__device__ __forceinline__ uint32_t comp_read_voxel(const ReadBox& B, int x, int y, int z)
{
    if (B.vox) return B.vox[(size_t)x + ((size_t)y + (size_t)z * (size_t)B.H) * (size_t)B.W];
    const size_t pc = (size_t)((x >> 3) + 1) + ((size_t)((y >> 3) + 1) + (size_t)((z >> 3) + 1) * (size_t)B.pby) * (size_t)B.pbx;
    const uint32_t ptr = ((const uint32_t*)B.bentry)[2u * pc] & 0xFFFFFFu;          // the entry's low word: pointer | open bits << 24
    if (ptr == 0u || ptr > B.bcap) return 0u;
    return B.bpool[(size_t)(ptr - 1u) * 512u + (size_t)((x & 7) | ((y & 7) << 3) | ((z & 7) << 6))];
}

__device__ __forceinline__ uint32_t comp_min(uint32_t a, uint32_t b) { return a < b ? a : b; }

// ---- pass 1 ------------------------------------------------------------------------------------------------------------------

#define VRT_COMP_EXT 1000u             // 10^3: the tile and a border of one voxel, x fastest

template <int CONN, bool SAME>
__global__ __launch_bounds__(64) void k_comp_tile(const CompJob J)
{
    __shared__ uint32_t s_lab[VRT_COMP_EXT];
    __shared__ uint8_t s_key[VRT_COMP_EXT];
    const uint32_t ti = blockIdx.x, lane = threadIdx.x;
    const uint32_t tx = ti % J.nt[0], ty = (ti / J.nt[0]) % J.nt[1], tz = ti / (J.nt[0] * J.nt[1]);
    for (uint32_t e = lane; e < VRT_COMP_EXT; e += 64u) { s_lab[e] = VRT_COMP_NONE; s_key[e] = 0; }
    __syncthreads();
    const uint32_t y = lane & 7u, z = lane >> 3, ry = ty * 8u + y, rz = tz * 8u + z, rx0 = tx * 8u;
    const bool row_in = ry < J.csize[1] && rz < J.csize[2];
    const uint32_t base = 1u + 10u * (y + 1u) + 100u * (z + 1u), lin0 = row_in ? comp_linear(rx0, ry, rz, J.csize) : 0u;
    uint32_t key[8], lab[8];
    bool any = false;
#pragma unroll
    for (uint32_t x = 0; x < 8u; x++) {
        const bool in = row_in && rx0 + x < J.csize[0];
        key[x] = in ? comp_key(J.match, comp_read_voxel(J.box, J.clo[0] + (int)(rx0 + x), J.clo[1] + (int)ry, J.clo[2] + (int)rz)) : 0u;
        lab[x] = key[x] != 0u ? lin0 + x : VRT_COMP_NONE;
        any = any || key[x] != 0u;
        s_lab[base + x] = lab[x];
        if (SAME) s_key[base + x] = (uint8_t)key[x];
    }
    __syncthreads();
    if (__ballot(any) != 0ull) {
        for (;;) {
            uint32_t nw[8];
            bool changed = false;
#pragma unroll
            for (uint32_t x = 0; x < 8u; x++) {
                uint32_t m = lab[x];
                if (key[x] != 0u) {
#pragma unroll
                    for (int o = 0; o < 27; o++) {
                        const int dx = o % 3 - 1, dy = (o / 3) % 3 - 1, dz = o / 9 - 1;
                        const int faces = (dx != 0) + (dy != 0) + (dz != 0);
                        if (faces == 0 || (CONN == VRT_COMP_CONN_FACES && faces != 1)) continue;
                        if (dy == 0 && dz == 0) continue;         // the row itself: in registers, below
                        const uint32_t e = (uint32_t)((int)(base + x) + dx + 10 * dy + 100 * dz);
                        const uint32_t l = s_lab[e];
                        if (!SAME || (uint32_t)s_key[e] == key[x]) m = comp_min(m, l);
                    }
                }
                nw[x] = m;
            }
#pragma unroll
            for (uint32_t x = 1; x < 8u; x++)
                if (key[x] != 0u && key[x] == key[x - 1u]) nw[x] = comp_min(nw[x], nw[x - 1u]);
#pragma unroll
            for (int x = 6; x >= 0; x--)
                if (key[x] != 0u && key[x] == key[x + 1]) nw[x] = comp_min(nw[x], nw[x + 1]);
#pragma unroll
            for (uint32_t x = 0; x < 8u; x++) changed = changed || nw[x] != lab[x];
            if (__ballot(changed) == 0ull) break;                 // the wave's vote: no label changed
            __syncthreads();
#pragma unroll
            for (uint32_t x = 0; x < 8u; x++) s_lab[base + x] = lab[x] = nw[x];
            __syncthreads();
        }
    }
    if (!row_in) return;
#pragma unroll
    for (uint32_t x = 0; x < 8u; x++)
        if (rx0 + x < J.csize[0]) J.labels[lin0 + x] = lab[x];
}

// ---- pass 2 ------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ uint32_t comp_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x, as far as this thread's loads show it; every step goes to a strictly smaller index
__device__ __forceinline__ uint32_t comp_find(const uint32_t* P, uint32_t x)
{
#if defined(VRT_COMP_DEBUG)
    uint32_t steps = 0u;
    const uint32_t bound = x;
#endif
    for (;;) {
        const uint32_t p = comp_load(P + x);
        if (p >= x) return x;                                     // a root (p == x; a word never exceeds its index)
        x = p;
#if defined(VRT_COMP_DEBUG)
        if (++steps > bound) return x;
#endif
    }
}

// a and b, two passing voxels, become one set: the larger root is linked under the smaller
__device__ __forceinline__ void comp_unite(uint32_t* P, uint32_t a, uint32_t b)
{
#if defined(VRT_COMP_DEBUG)
    uint64_t turns = 0u;
    const uint64_t bound = (uint64_t)a + b;
#endif
    for (;;) {
        a = comp_find(P, a);
        b = comp_find(P, b);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = atomicMin(P + a, b);                 // device scope
        if (old == a) return;                                     // a was a root and is linked
        a = old;                                                  // a had been linked under old < a: old and b are still to unite
#if defined(VRT_COMP_DEBUG)
        if (++turns > bound) return;
#endif
    }
}

template <int CONN>
__global__ __launch_bounds__(256) void k_comp_seam(const CompJob J, uint32_t n)
{
    const uint32_t L = blockIdx.x * 256u + threadIdx.x;
    if (L >= n) return;
    const uint32_t rx = L % J.csize[0], ry = (L / J.csize[0]) % J.csize[1], rz = L / (J.csize[0] * J.csize[1]);
    const uint32_t ex = rx & 7u, ey = ry & 7u, ez = rz & 7u;
    if (ex != 0u && ex != 7u && ey != 0u && ey != 7u && ez != 0u && ez != 7u) return;      // every neighbour lies in the voxel's own tile
    if (J.labels[L] == VRT_COMP_NONE) return;
    const bool same = J.match == VRT_COMP_MATCH_SAME;
    const uint32_t id = same ? comp_read_voxel(J.box, J.clo[0] + (int)rx, J.clo[1] + (int)ry, J.clo[2] + (int)rz) : 0u;
    const uint32_t nd = CONN == VRT_COMP_CONN_FACES ? 3u : 13u;
    for (uint32_t k = 0; k < nd; k++) {
        int d[3];
        comp_forward(CONN, k, d);
        const int nx = (int)rx + d[0], ny = (int)ry + d[1], nz = (int)rz + d[2];
        if (nx < 0 || nx >= (int)J.csize[0] || ny < 0 || ny >= (int)J.csize[1] || nz < 0 || nz >= (int)J.csize[2]) continue;
        if ((nx >> 3) == (int)(rx >> 3) && (ny >> 3) == (int)(ry >> 3) && (nz >> 3) == (int)(rz >> 3)) continue;    // pass 1 joined them
        const uint32_t M = comp_linear((uint32_t)nx, (uint32_t)ny, (uint32_t)nz, J.csize);
        if (J.labels[M] == VRT_COMP_NONE) continue;               // (a word that is not NONE never becomes it, and the other way round)
        if (same && comp_read_voxel(J.box, J.clo[0] + nx, J.clo[1] + ny, J.clo[2] + nz) != id) continue;
        comp_unite(J.labels, L, M);
    }
}

// ---- passes 3 and 4 ------------------------------------------------------------------------------------------------------------

// segment g of the clipped bounds -> this lane's offset and linear index; in_row: the lane lies in the row.  false: no such segment
__device__ __forceinline__ bool comp_lane(const uint32_t size[3], uint32_t g, uint32_t lane, uint32_t& bx, uint32_t& by, uint32_t& bz, bool& in_row)
{
    const uint32_t spr = list_segments_per_row(size[0]);
    if (g >= spr * size[1] * size[2]) return false;
    const uint32_t row = g / spr;
    bx = (g - row * spr) * VRT_LIST_SEGMENT + lane;
    bz = row / size[1];
    by = row - bz * size[1];
    in_row = bx < size[0];
    return true;
}

__global__ __launch_bounds__(256) void k_comp_flatten(const CompJob J, uint32_t* __restrict__ work)
{
    const uint32_t lane = threadIdx.x & 63u, g = blockIdx.x * 4u + (threadIdx.x >> 6);
    uint32_t bx, by, bz;
    bool in_row;
    if (!comp_lane(J.csize, g, lane, bx, by, bz, in_row)) return;
    bool root = false;
    if (in_row) {
        const uint32_t L = comp_linear(bx, by, bz, J.csize), p = J.labels[L];
        if (p != VRT_COMP_NONE) {
            const uint32_t r = comp_find(J.labels, L);
            if (r != p) J.labels[L] = r;                          // an ancestor for a parent: any reader of the old or the new word ends at r
            root = r == L;
        }
    }
    const uint64_t mask = __ballot(root);
    if (lane == 0u) work[g] = (uint32_t)__popcll(mask);
}

__global__ __launch_bounds__(256) void k_comp_number(const CompJob J, const uint32_t* __restrict__ work)
{
    const uint32_t lane = threadIdx.x & 63u, g = blockIdx.x * 4u + (threadIdx.x >> 6);
    uint32_t bx, by, bz;
    bool in_row;
    if (!comp_lane(J.csize, g, lane, bx, by, bz, in_row)) return;
    const uint32_t L = in_row ? comp_linear(bx, by, bz, J.csize) : 0u;
    const bool root = in_row && J.labels[L] == L;
    const uint64_t mask = __ballot(root);
    if (!root) return;
    const uint32_t k = work[g] + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
    if (k >= J.ncomp) return;
    CompStat t;
    t.root = L; t.id = comp_read_voxel(J.box, J.clo[0] + (int)bx, J.clo[1] + (int)by, J.clo[2] + (int)bz);
    t.count = 0u; t.selected = 0u;
    for (int a = 0; a < 3; a++) { t.mn[a] = 0xFFFFFFFFu; t.mx[a] = 0u; }
    J.table[k] = t;
    J.labels[L] = VRT_COMP_NUMBERED | k;
}

// ---- pass 5 ------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(64) void k_comp_measure(const CompJob J, uint32_t n)
{
    const uint32_t ti = blockIdx.x, lane = threadIdx.x;
    const uint32_t tx = ti % J.nt[0], ty = (ti / J.nt[0]) % J.nt[1], tz = ti / (J.nt[0] * J.nt[1]);
    const uint32_t y = lane & 7u, z = lane >> 3, ry = ty * 8u + y, rz = tz * 8u + z, rx0 = tx * 8u;
    const bool row_in = ry < J.csize[1] && rz < J.csize[2];
    const uint32_t lin0 = row_in ? comp_linear(rx0, ry, rz, J.csize) : 0u;
    uint32_t num[8], todo = 0u;
#pragma unroll
    for (uint32_t x = 0; x < 8u; x++) {
        num[x] = VRT_COMP_NONE;
        if (!row_in || rx0 + x >= J.csize[0]) continue;
        uint32_t v = J.labels[lin0 + x];
        if (v == VRT_COMP_NONE) continue;
        if ((v & VRT_COMP_NUMBERED) == 0u) {                      // a parent: the root's word holds the number, and no one rewrites a root's word here
            v = v < n ? J.labels[v] : VRT_COMP_NONE;
            if (v == VRT_COMP_NONE || (v & VRT_COMP_NUMBERED) == 0u) continue;
            J.labels[lin0 + x] = v;
        }
        num[x] = v & ~VRT_COMP_NUMBERED;
        todo |= 1u << x;
    }
    // one component of the tile a turn: the lowest lane with a voxel left names it
    for (;;) {
        const uint64_t left = __ballot(todo != 0u);
        if (left == 0ull) break;
        const uint32_t first = todo != 0u ? (uint32_t)__builtin_ctz(todo) : 0u;
        uint32_t mine = num[0];
#pragma unroll
        for (uint32_t x = 1; x < 8u; x++) mine = first == x ? num[x] : mine;
        const uint32_t k = (uint32_t)__shfl((int)mine, (int)__builtin_ctzll(left));
        uint32_t xm = 0u;
#pragma unroll
        for (uint32_t x = 0; x < 8u; x++)
            if (((todo >> x) & 1u) != 0u && num[x] == k) xm |= 1u << x;
        todo &= ~xm;
        uint64_t rows = 0ull;
        uint32_t count = 0u, xs = 0u;
#pragma unroll
        for (uint32_t x = 0; x < 8u; x++) {
            const uint64_t b = __ballot(((xm >> x) & 1u) != 0u);
            rows |= b;
            count += (uint32_t)__popcll(b);
            if (b != 0ull) xs |= 1u << x;
        }
        if (k >= J.ncomp || rows == 0ull) continue;               // (wave-uniform)
        uint32_t ys = (uint32_t)(rows | (rows >> 32));
        ys |= ys >> 16; ys |= ys >> 8; ys &= 0xFFu;
        const uint32_t mn[3] = {rx0 + (uint32_t)__builtin_ctz(xs), ty * 8u + (uint32_t)__builtin_ctz(ys), tz * 8u + ((uint32_t)__builtin_ctzll(rows) >> 3)};
        const uint32_t mx[3] = {rx0 + 31u - (uint32_t)__builtin_clz(xs), ty * 8u + 31u - (uint32_t)__builtin_clz(ys), tz * 8u + ((63u - (uint32_t)__builtin_clzll(rows)) >> 3)};
        CompStat* const t = J.table + k;
        if (lane == 0u) atomicAdd(&t->count, count);
        else if (lane < 4u) atomicMin(&t->mn[lane - 1u], lane == 1u ? mn[0] : lane == 2u ? mn[1] : mn[2]);
        else if (lane < 7u) atomicMax(&t->mx[lane - 4u], lane == 4u ? mx[0] : lane == 5u ? mx[1] : mx[2]);
    }
}

// ---- pass 6 and the filter -------------------------------------------------------------------------------------------------------

__device__ __forceinline__ unsigned long long comp_wave_max(unsigned long long v)
{
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = ((unsigned long long)(uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d) << 32) | (unsigned long long)(uint32_t)__shfl_xor((int)(uint32_t)v, d);
        v = o > v ? o : v;
    }
    return v;
}

__device__ __forceinline__ unsigned long long comp_wave_sum(unsigned long long v)
{
    for (int d = 32; d >= 1; d >>= 1)
        v += ((unsigned long long)(uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d) << 32) | (unsigned long long)(uint32_t)__shfl_xor((int)(uint32_t)v, d);
    return v;
}

__global__ __launch_bounds__(256) void k_comp_summary(const CompJob J, CompSummary* __restrict__ sum)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    const bool in = k < J.ncomp;
    const uint32_t count = in ? J.table[k].count : 0u;
    const unsigned long long best = comp_wave_max(in ? comp_largest_key(count, k) : 0ull), total = comp_wave_sum(count);
    if ((threadIdx.x & 63u) == 0u && total != 0ull) {
        atomicMax(&sum->largest, best);
        atomicAdd(&sum->voxels, total);
    }
}

__global__ __launch_bounds__(256) void k_comp_select(const CompJob J, const CompFilter F, CompSummary* __restrict__ sum)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    bool sel = false;
    uint32_t count = 0u;
    if (k < J.ncomp) {
        const CompStat t = J.table[k];
        sel = comp_selected(t.count, comp_faces(t.mn, t.mx, J.csize), k == F.largest, F.min_voxels, F.max_voxels, F.faces_all, F.faces_none, F.flags);
        J.table[k].selected = sel ? 1u : 0u;
        count = sel ? t.count : 0u;
    }
    const unsigned long long comps = (unsigned long long)__popcll(__ballot(sel)), voxels = comp_wave_sum(count);
    if ((threadIdx.x & 63u) == 0u && comps != 0ull) {
        atomicAdd(&sum->sel_components, comps);
        atomicAdd(&sum->sel_voxels, voxels);
    }
}

// is the voxel at offset (bx, by, bz) of J.box, which lies inside the clipped bounds, in a selected component?
__device__ __forceinline__ bool comp_inside(const CompJob& J, uint32_t bx, uint32_t by, uint32_t bz)
{
    const uint32_t rx = (uint32_t)(J.box.lo[0] - J.clo[0]) + bx, ry = (uint32_t)(J.box.lo[1] - J.clo[1]) + by, rz = (uint32_t)(J.box.lo[2] - J.clo[2]) + bz;
    if (rx >= J.csize[0] || ry >= J.csize[1] || rz >= J.csize[2]) return false;
    const uint32_t v = J.labels[comp_linear(rx, ry, rz, J.csize)];
    if (v == VRT_COMP_NONE || (v & VRT_COMP_NUMBERED) == 0u) return false;
    const uint32_t k = v & ~VRT_COMP_NUMBERED;
    return k < J.ncomp && J.table[k].selected != 0u;
}

// four waves per block, a segment each; J.box is the clipped bounds
__global__ __launch_bounds__(256) void k_comp_extent(const CompJob J, BrushRecord* __restrict__ rec)
{
    __shared__ uint32_t s_count;
    __shared__ int32_t s_mn[3], s_mx[3];
    if (threadIdx.x < 3u) { s_mn[threadIdx.x] = INT32_MAX; s_mx[threadIdx.x] = INT32_MIN; }
    if (threadIdx.x == 0u) s_count = 0u;
    __syncthreads();
    const ReadBox& B = J.box;
    const uint32_t lane = threadIdx.x & 63u, g = blockIdx.x * 4u + (threadIdx.x >> 6);
    uint32_t bx, by, bz;
    bool in_row;
    if (comp_lane(B.size, g, lane, bx, by, bz, in_row)) {
        const int x = B.lo[0] + (int)bx, y = B.lo[1] + (int)by, z = B.lo[2] + (int)bz;
        const bool changed = in_row && comp_inside(J, bx, by, bz) && comp_read_voxel(B, x, y, z) != J.id;
        const uint64_t cmask = __ballot(changed);
        if (cmask != 0ull && lane == 0u) {
            atomicAdd(&s_count, (uint32_t)__popcll(cmask));
            atomicMin(&s_mn[0], x + (int)__builtin_ctzll(cmask)); atomicMax(&s_mx[0], x + 63 - (int)__builtin_clzll(cmask));
            atomicMin(&s_mn[1], y); atomicMax(&s_mx[1], y);
            atomicMin(&s_mn[2], z); atomicMax(&s_mx[2], z);
        }
    }
    __syncthreads();
    if (s_count == 0u) return;
    if (threadIdx.x == 0u) { atomicAdd(&rec->changed, (unsigned long long)s_count); atomicOr(&rec->ids[J.id >> 5], 1u << (J.id & 31u)); }
    if (threadIdx.x < 3u) { atomicMin(&rec->mn[threadIdx.x], s_mn[threadIdx.x]); atomicMax(&rec->mx[threadIdx.x], s_mx[threadIdx.x]); }
}

// J.box is the tight box of the changed voxels
__global__ __launch_bounds__(256) void k_comp_compose(const CompJob J, uint8_t* __restrict__ ids)
{
    const ReadBox& B = J.box;
    const uint32_t lane = threadIdx.x & 63u, g = blockIdx.x * 4u + (threadIdx.x >> 6);
    uint32_t bx, by, bz;
    bool in_row;
    if (!comp_lane(B.size, g, lane, bx, by, bz, in_row) || !in_row) return;
    const uint32_t nw = comp_inside(J, bx, by, bz) ? J.id : comp_read_voxel(B, B.lo[0] + (int)bx, B.lo[1] + (int)by, B.lo[2] + (int)bz);
    ids[read_box_index(bx, by, bz, B.size)] = (uint8_t)nw;
}

struct CompBox { uint32_t off[3], size[3]; };

// the box at offset B.off of the clipped bounds, B.size large and inside them
__global__ __launch_bounds__(256) void k_comp_labels(const CompJob J, const CompBox B, uint32_t* __restrict__ out)
{
    const uint32_t lane = threadIdx.x & 63u, g = blockIdx.x * 4u + (threadIdx.x >> 6);
    uint32_t bx, by, bz;
    bool in_row;
    if (!comp_lane(B.size, g, lane, bx, by, bz, in_row) || !in_row) return;
    const uint32_t rx = B.off[0] + bx, ry = B.off[1] + by, rz = B.off[2] + bz;
    uint32_t v = VRT_COMP_NONE;
    if (rx < J.csize[0] && ry < J.csize[1] && rz < J.csize[2]) v = J.labels[comp_linear(rx, ry, rz, J.csize)];
    out[read_box_index(bx, by, bz, B.size)] = v == VRT_COMP_NONE ? v : v & ~VRT_COMP_NUMBERED;
}

// ---- launchers -----------------------------------------------------------------------------------------------------------------

static uint32_t comp_voxels(const CompJob& j) { return j.csize[0] * j.csize[1] * j.csize[2]; }
static uint32_t comp_tile_count(const CompJob& j) { return j.nt[0] * j.nt[1] * j.nt[2]; }
static uint32_t comp_segment_blocks(const uint32_t size[3]) { return (list_segments_per_row(size[0]) * size[1] * size[2] + 3u) / 4u; }

hipError_t launch_comp_tile(const CompJob& j, hipStream_t s)
{
    const dim3 grid(comp_tile_count(j)), block(64);
    const bool same = j.match == VRT_COMP_MATCH_SAME;
    if (j.connectivity == VRT_COMP_CONN_FACES) {
        if (same) hipLaunchKernelGGL((k_comp_tile<VRT_COMP_CONN_FACES, true>), grid, block, 0, s, j);
        else      hipLaunchKernelGGL((k_comp_tile<VRT_COMP_CONN_FACES, false>), grid, block, 0, s, j);
    } else if (j.connectivity == VRT_COMP_CONN_CORNERS) {
        if (same) hipLaunchKernelGGL((k_comp_tile<VRT_COMP_CONN_CORNERS, true>), grid, block, 0, s, j);
        else      hipLaunchKernelGGL((k_comp_tile<VRT_COMP_CONN_CORNERS, false>), grid, block, 0, s, j);
    } else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_comp_seam(const CompJob& j, hipStream_t s)
{
    const uint32_t n = comp_voxels(j);
    const dim3 grid((n + 255u) / 256u), block(256);
    switch (j.connectivity) {
    case VRT_COMP_CONN_FACES:   hipLaunchKernelGGL(k_comp_seam<VRT_COMP_CONN_FACES>, grid, block, 0, s, j, n); break;
    case VRT_COMP_CONN_CORNERS: hipLaunchKernelGGL(k_comp_seam<VRT_COMP_CONN_CORNERS>, grid, block, 0, s, j, n); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_comp_flatten(const CompJob& j, uint32_t* work, hipStream_t s)
{
    hipLaunchKernelGGL(k_comp_flatten, dim3(comp_segment_blocks(j.csize)), dim3(256), 0, s, j, work);
    return hipGetLastError();
}

hipError_t launch_comp_number(const CompJob& j, const uint32_t* work, hipStream_t s)
{
    hipLaunchKernelGGL(k_comp_number, dim3(comp_segment_blocks(j.csize)), dim3(256), 0, s, j, work);
    return hipGetLastError();
}

hipError_t launch_comp_measure(const CompJob& j, hipStream_t s)
{
    hipLaunchKernelGGL(k_comp_measure, dim3(comp_tile_count(j)), dim3(64), 0, s, j, comp_voxels(j));
    return hipGetLastError();
}

hipError_t launch_comp_summary(const CompJob& j, CompSummary* sum, hipStream_t s)
{
    if (j.ncomp == 0u) return hipSuccess;
    hipLaunchKernelGGL(k_comp_summary, dim3((j.ncomp + 255u) / 256u), dim3(256), 0, s, j, sum);
    return hipGetLastError();
}

hipError_t launch_comp_select(const CompJob& j, const CompFilter& f, CompSummary* sum, hipStream_t s)
{
    if (j.ncomp == 0u) return hipSuccess;
    hipLaunchKernelGGL(k_comp_select, dim3((j.ncomp + 255u) / 256u), dim3(256), 0, s, j, f, sum);
    return hipGetLastError();
}

hipError_t launch_comp_extent(const CompJob& j, BrushRecord* rec, hipStream_t s)
{
    hipLaunchKernelGGL(k_comp_extent, dim3(comp_segment_blocks(j.box.size)), dim3(256), 0, s, j, rec);
    return hipGetLastError();
}

hipError_t launch_comp_compose(const CompJob& j, uint8_t* ids, hipStream_t s)
{
    hipLaunchKernelGGL(k_comp_compose, dim3(comp_segment_blocks(j.box.size)), dim3(256), 0, s, j, ids);
    return hipGetLastError();
}

hipError_t launch_comp_labels(const CompJob& j, const int32_t lo[3], const uint32_t size[3], uint32_t* out, hipStream_t s)
{
    CompBox b;
    for (int a = 0; a < 3; a++) { b.off[a] = (uint32_t)(lo[a] - j.clo[a]); b.size[a] = size[a]; }
    hipLaunchKernelGGL(k_comp_labels, dim3(comp_segment_blocks(size)), dim3(256), 0, s, j, b, out);
    return hipGetLastError();
}

} // namespace vrt
