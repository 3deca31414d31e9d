// vrt_flood.h -- which voxels a flood fill selects (vrt_scene_flood) and how the device finds them.  Plain integer arithmetic,
// compiled for the device (vrt_flood.hip), the host (vrt_api_edit.hip) and the tests (tests/native/flood_host.cpp,
// flood_fuzz.cpp, held against a plain BFS in Python integers, tests/flood_reference.py).
//
// DEFINITION.  The BOUNDS are [lo, lo + size) in voxels; lo may be negative, every size in 1..2^30.  They are cut to the volume
// with brush_clip (vrt_brush.h).  Bounds wholly outside the volume, or a seed outside the clipped bounds, select nothing and are
// no error.  A clipped side above VRT_FLOOD_MAX_SIDE = 512 is refused: flood in parts.
//   PREDICATE   VRT_FLOOD_MATCH_SAME   a voxel passes iff its id equals the id of the seed voxel (0 included: the cavity fill)
//               VRT_FLOOD_MATCH_SOLID  a voxel passes iff its id != 0
//   REGION      the connected component of the seed in the graph of the passing voxels OF THE CLIPPED BOUNDS, two voxels being
//               joined when they share a face (VRT_FLOOD_CONN_FACES = 6) or a face, an edge or a corner (VRT_FLOOD_CONN_CORNERS =
//               26).  A seed that does not pass (an empty seed under SOLID) has the empty region.
//   EDIT        every voxel of the region becomes `id`; `changed` counts those whose id differed, the tight box holds those only.
//
// LAYOUT.  The clipped bounds are cut into TILES of 8^3 voxels counted from the CLIPPED lo (not from the brick grid): the voxel
// at offset (rx, ry, rz) from the clipped lo lies in tile (rx >> 3, ry >> 3, rz >> 3); there are nt[a] = ceil(csize[a] / 8) <= 64
// tiles along axis a, tile (tx, ty, tz) has the TILE INDEX
//     ti = tx + (ty + tz * nt[1]) * nt[0]                                                           (flood_tile_index)
// Two MASKS over the tiles, PASSABLE and REACHED, hold one bit per voxel: 64 bytes per tile and mask, the byte
//     ti * 64 + (ry & 7) + 8 * (rz & 7)                                                              (flood_mask_byte)
// is the row (y, z) of the tile and its bit rx & 7 the voxel.  Bits of a last tile that lie beyond the clipped bounds are 0 in
// both masks.  Two masks over bounds of 512^3 are 2 x 16 MiB.
//
// ONE TILE STEP.  A tile is relaxed on its EXTENDED rows: ext[(y + 1) + 10 * (z + 1)], y and z in -1..8, is a row of ten bits
// of the reached mask, bit x + 1 being the voxel at x in -1..8 of the tile's own coordinates (flood_ext_row gathers it; what
// lies in a neighbour tile is the SHELL, what lies outside the bounds is 0; under 6-connectivity only the six faces of the
// shell are gathered, under 26 its edges and corners too).  flood_row_relax gives what one row of the tile becomes,
//     reached |= dilate(reached) & passable
// and flood_tile_relax repeats it over the 64 rows until no row changes.  The shell does not change during a step.  The kernel
// runs the same two functions, a lane per row, and ends its loop by a wave vote.
//
// ROUNDS AND THE WAKE-UP INVARIANT.  A round runs one step on every ACTIVE tile.  The activity flags are double-buffered: round
// k reads and clears buffer k & 1 and sets flags in buffer (k + 1) & 1.  The seed's bit counts as gained before round 0: the
// seed's tile and the neighbour tiles that can see the seed (flood_seed_tiles) are active in round 0.  A tile that
// gained bits sets, for the next round, the flag of every neighbour tile that can see one of the gained bits
// (flood_wake_mask: a gained bit on face x = 7 wakes the neighbour at +x, and under 26-connectivity a bit on an edge or in a
// corner wakes the tiles across that edge or corner too).  The invariant the code is held to:
//     a tile may be skipped in a round only if no tile adjacent to it under the chosen connectivity has gained a bit that it
//     can see since it last ran.
// A tile that ran in round k beside a neighbour that gained bits in the same round may or may not have seen them; the neighbour
// wakes it for round k + 1 either way, where it sees them all (a round is a kernel launch).  The rounds end when a round sets no
// flag.
//
// SCHEDULE INDEPENDENCE.  Propagation is monotone: bits are only ever set, and a set bit never stops another from being set.
// So whatever the order in which tiles run, and whichever of a neighbour's bits a tile happens to see, the fixed point is the
// same: the component of the seed.  The kernels therefore need no ordering among the waves of a round -- plain byte stores to a
// tile's own rows, plain stores of 1 to flags -- and no wave ever waits for another.
//
// THE LOOP BOUND.  Every round but the last gains at least one bit, so there are at most (voxels of the clipped bounds) + 1 of
// them (flood_round_bound); a host loop that exceeds it reports an internal error instead of running on.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define VRT_FLOOD_HD __host__ __device__ inline
#else
#define VRT_FLOOD_HD inline
#endif

// (include/vrt.h has the same values for the C-ABI; vrt_api_edit.hip asserts that they agree)
#define VRT_FLOOD_MATCH_SAME 0
#define VRT_FLOOD_MATCH_SOLID 1
#define VRT_FLOOD_CONN_FACES 6
#define VRT_FLOOD_CONN_CORNERS 26
#define VRT_FLOOD_FLAG_MEASURE 1u

#define VRT_FLOOD_MAX_SIDE 512u           // voxels, of the clipped bounds
#define VRT_FLOOD_MAX_SIZE (1u << 30)     // of the bounds as given
#define VRT_FLOOD_TILE 8u
#define VRT_FLOOD_TILE_BYTES 64u          // per tile and mask
#define VRT_FLOOD_EXT_ROWS 100u           // 10 x 10 extended rows of ten bits

namespace vrt {

VRT_FLOOD_HD bool flood_args_ok(int32_t match, int32_t connectivity, uint32_t flags, const uint32_t size[3])
{
    if (match != VRT_FLOOD_MATCH_SAME && match != VRT_FLOOD_MATCH_SOLID) return false;
    if (connectivity != VRT_FLOOD_CONN_FACES && connectivity != VRT_FLOOD_CONN_CORNERS) return false;
    if (flags & ~VRT_FLOOD_FLAG_MEASURE) return false;
    for (int a = 0; a < 3; a++)
        if (size[a] < 1u || size[a] > VRT_FLOOD_MAX_SIZE) return false;
    return true;
}

// the clipped bounds' sides as the masks allow them
VRT_FLOOD_HD bool flood_sides_ok(const uint32_t csize[3])
{
    return csize[0] <= VRT_FLOOD_MAX_SIDE && csize[1] <= VRT_FLOOD_MAX_SIDE && csize[2] <= VRT_FLOOD_MAX_SIDE;
}

VRT_FLOOD_HD bool flood_seed_inside(const int32_t seed[3], const int32_t clo[3], const uint32_t csize[3])
{
    for (int a = 0; a < 3; a++)
        if ((int64_t)seed[a] < (int64_t)clo[a] || (int64_t)seed[a] >= (int64_t)clo[a] + (int64_t)csize[a]) return false;
    return true;
}

VRT_FLOOD_HD bool flood_passes(int32_t match, uint32_t id, uint32_t seed_id) { return match == VRT_FLOOD_MATCH_SAME ? id == seed_id : id != 0u; }

VRT_FLOOD_HD void flood_tiles(const uint32_t csize[3], uint32_t nt[3])
{
    for (int a = 0; a < 3; a++) nt[a] = (csize[a] + VRT_FLOOD_TILE - 1u) / VRT_FLOOD_TILE;
}

VRT_FLOOD_HD size_t flood_tile_count(const uint32_t nt[3]) { return (size_t)nt[0] * (size_t)nt[1] * (size_t)nt[2]; }

VRT_FLOOD_HD size_t flood_tile_index(uint32_t tx, uint32_t ty, uint32_t tz, const uint32_t nt[3])
{
    return (size_t)tx + ((size_t)ty + (size_t)tz * (size_t)nt[1]) * (size_t)nt[0];
}

// the mask byte and bit of the voxel at offset (rx, ry, rz) from the clipped lo
VRT_FLOOD_HD size_t flood_mask_byte(uint32_t rx, uint32_t ry, uint32_t rz, const uint32_t nt[3])
{
    return flood_tile_index(rx >> 3, ry >> 3, rz >> 3, nt) * VRT_FLOOD_TILE_BYTES + (size_t)((ry & 7u) | ((rz & 7u) << 3));
}
VRT_FLOOD_HD uint32_t flood_mask_bit(uint32_t rx) { return rx & 7u; }

// rounds the host loop may run: voxels of the clipped bounds + 1
VRT_FLOOD_HD uint64_t flood_round_bound(const uint32_t csize[3]) { return (uint64_t)csize[0] * (uint64_t)csize[1] * (uint64_t)csize[2] + 1ull; }

// extended row e = (y + 1) + 10 * (z + 1) of tile (tx, ty, tz), from the reached mask
VRT_FLOOD_HD uint32_t flood_ext_row(int connectivity, const uint8_t* reached, const uint32_t nt[3], uint32_t tx, uint32_t ty, uint32_t tz, uint32_t e)
{
    const uint32_t ey = e % 10u, ez = e / 10u;
    const int dy = ey == 0u ? -1 : ey == 9u ? 1 : 0, dz = ez == 0u ? -1 : ez == 9u ? 1 : 0;
    if (connectivity == VRT_FLOOD_CONN_FACES && dy != 0 && dz != 0) return 0u;
    const int64_t sy = (int64_t)ty + dy, sz = (int64_t)tz + dz;
    if (sy < 0 || sy >= (int64_t)nt[1] || sz < 0 || sz >= (int64_t)nt[2]) return 0u;
    const size_t row = (size_t)(((ey + 7u) & 7u) | (((ez + 7u) & 7u) << 3));            // ey - 1 and ez - 1, wrapped into the tile they lie in
    uint32_t r = (uint32_t)reached[flood_tile_index(tx, (uint32_t)sy, (uint32_t)sz, nt) * VRT_FLOOD_TILE_BYTES + row] << 1;
    if (connectivity == VRT_FLOOD_CONN_FACES && (dy != 0 || dz != 0)) return r;
    if (tx > 0u) r |= (uint32_t)reached[flood_tile_index(tx - 1u, (uint32_t)sy, (uint32_t)sz, nt) * VRT_FLOOD_TILE_BYTES + row] >> 7;
    if (tx + 1u < nt[0]) r |= ((uint32_t)reached[flood_tile_index(tx + 1u, (uint32_t)sy, (uint32_t)sz, nt) * VRT_FLOOD_TILE_BYTES + row] & 1u) << 9;
    return r;
}

// what row (y, z) of the tile, y and z in 0..7, becomes: its reached bits | the dilation of the extended rows & its passable bits
VRT_FLOOD_HD uint32_t flood_row_relax(int connectivity, const uint32_t* ext, uint32_t y, uint32_t z, uint32_t passable)
{
    const uint32_t* c = ext + (y + 1u) + 10u * (z + 1u);
    const uint32_t r = c[0];
    uint32_t d;
    if (connectivity == VRT_FLOOD_CONN_FACES) d = (r << 1) | (r >> 1) | c[-1] | c[1] | c[-10] | c[10];
    else {
        const uint32_t u = c[-11] | c[-10] | c[-9] | c[-1] | r | c[1] | c[9] | c[10] | c[11];
        d = u | (u << 1) | (u >> 1);
    }
    return r | (d & (passable << 1));
}

// one tile step on the host: the 64 rows to their fixed point under a shell that stays.  ext is updated in place; true: a bit was gained
VRT_FLOOD_HD bool flood_tile_relax(int connectivity, const uint8_t passable[64], uint32_t ext[VRT_FLOOD_EXT_ROWS])
{
    bool gained = false;
    for (;;) {
        uint32_t nw[64];
        bool changed = false;
        for (uint32_t l = 0; l < 64u; l++) {
            nw[l] = flood_row_relax(connectivity, ext, l & 7u, l >> 3, passable[l]);
            changed = changed || nw[l] != ext[(l & 7u) + 1u + 10u * ((l >> 3) + 1u)];
        }
        if (!changed) return gained;
        gained = true;
        for (uint32_t l = 0; l < 64u; l++) ext[(l & 7u) + 1u + 10u * ((l >> 3) + 1u)] = nw[l];
    }
}

// The neighbour tiles that can see a bit row (y, z) gained, before -> after (bytes of the reached mask): bit
// (dx + 1) + 3 * (dy + 1) + 9 * (dz + 1) for the tile at offset (dx, dy, dz).  The OR over a tile's rows is the set it wakes.
VRT_FLOOD_HD uint32_t flood_wake_mask(int connectivity, uint32_t before, uint32_t after, uint32_t y, uint32_t z)
{
    const uint32_t g = after & ~before & 0xFFu;
    if (g == 0u) return 0u;
    uint32_t m = 0u;
    for (int dz = -1; dz <= 1; dz++) for (int dy = -1; dy <= 1; dy++) for (int dx = -1; dx <= 1; dx++) {
        const int faces = (dx != 0) + (dy != 0) + (dz != 0);
        if (faces == 0 || (connectivity == VRT_FLOOD_CONN_FACES && faces != 1)) continue;
        const bool sx = dx == 0 || (g & (dx > 0 ? 0x80u : 0x01u)) != 0u;
        const bool sy = dy == 0 || y == (dy > 0 ? 7u : 0u), sz = dz == 0 || z == (dz > 0 ? 7u : 0u);
        if (sx && sy && sz) m |= 1u << ((dx + 1) + 3 * (dy + 1) + 9 * (dz + 1));
    }
    return m;
}

// The tiles active in round 0: the seed's (bit 13, offset (0, 0, 0)) and the neighbours that can see the seed's bit, as flood_wake_mask
// numbers them.  (rx, ry, rz): the seed's offset from the clipped lo.
VRT_FLOOD_HD uint32_t flood_seed_tiles(int connectivity, uint32_t rx, uint32_t ry, uint32_t rz)
{
    return (1u << 13) | flood_wake_mask(connectivity, 0u, 1u << flood_mask_bit(rx), ry & 7u, rz & 7u);
}

} // namespace vrt
