// Host build of csrc/vrt_flood.h for the tests (tests/flood_native.py, flood_fuzz.cpp): the header's functions one by one, and
// the whole tiled algorithm -- masks, extended rows, tile steps, activity flags, rounds -- run on the host in a chosen tile
// order, as the device runs it in whatever order its waves happen to take.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../voxel-raytracing_amd/csrc/vrt_brush.h"
#include "../../voxel-raytracing_amd/csrc/vrt_flood.h"

using namespace vrt;

namespace {

uint32_t lcg(uint64_t& s) { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }

}

// order: 0 forward, 1 reverse, 2 a new random permutation every round (seeded by rng), 3 forward, every tile of a round seeing
// the reached mask as it was when the round began (the most a device tile can miss).
// res: region, region_lo[3], region_size[3], seed_id, changed, lo[3], size[3], rounds.  vol (x fastest) is rewritten unless
// measure.  Returns 0, 1 (an argument is refused) or 6 (the loop bound was exceeded).
extern "C" int flood_run_c(const int32_t dim[3], uint8_t* vol, const int32_t seed[3], const int32_t lo[3], const uint32_t size[3], int32_t match,
                           int32_t conn, uint32_t flags, uint32_t id, int order, uint64_t rng, int64_t res[16])
{
    memset(res, 0, 16 * sizeof(int64_t));
    if (!flood_args_ok(match, conn, flags, size)) return 1;
    int64_t l[3], h[3];
    int32_t clo[3];
    uint32_t cs[3], nt[3];
    for (int a = 0; a < 3; a++) { l[a] = lo[a]; h[a] = (int64_t)lo[a] + size[a]; }
    const bool any = brush_clip(l, h, dim, clo, cs);
    if (any && !flood_sides_ok(cs)) return 1;
    if (!any || !flood_seed_inside(seed, clo, cs)) return 0;
    flood_tiles(cs, nt);
    const size_t ntiles = flood_tile_count(nt);
    std::vector<uint8_t> passable(ntiles * 64, 0), reached(ntiles * 64, 0), snap;
    std::vector<uint8_t> act[2] = {std::vector<uint8_t>(ntiles, 0), std::vector<uint8_t>(ntiles, 0)};
    auto at = [&](uint32_t rx, uint32_t ry, uint32_t rz) -> uint8_t& {
        return vol[(size_t)(clo[0] + (int)rx) + ((size_t)(clo[1] + (int)ry) + (size_t)(clo[2] + (int)rz) * (size_t)dim[1]) * (size_t)dim[0]];
    };
    const uint32_t sr[3] = {(uint32_t)(seed[0] - clo[0]), (uint32_t)(seed[1] - clo[1]), (uint32_t)(seed[2] - clo[2])};
    const uint32_t seed_id = at(sr[0], sr[1], sr[2]);
    for (uint32_t z = 0; z < cs[2]; z++) for (uint32_t y = 0; y < cs[1]; y++) for (uint32_t x = 0; x < cs[0]; x++)
        if (flood_passes(match, at(x, y, z), seed_id)) passable[flood_mask_byte(x, y, z, nt)] |= (uint8_t)(1u << flood_mask_bit(x));
    if (flood_passes(match, seed_id, seed_id)) {
        reached[flood_mask_byte(sr[0], sr[1], sr[2], nt)] = (uint8_t)(1u << flood_mask_bit(sr[0]));
        const uint32_t tiles = flood_seed_tiles(conn, sr[0], sr[1], sr[2]);
        for (uint32_t o = 0; o < 27; o++) {
            const int nx = (int)(sr[0] >> 3) + (int)(o % 3) - 1, ny = (int)(sr[1] >> 3) + (int)((o / 3) % 3) - 1, nz = (int)(sr[2] >> 3) + (int)(o / 9) - 1;
            if (((tiles >> o) & 1u) && nx >= 0 && nx < (int)nt[0] && ny >= 0 && ny < (int)nt[1] && nz >= 0 && nz < (int)nt[2])
                act[0][flood_tile_index((uint32_t)nx, (uint32_t)ny, (uint32_t)nz, nt)] = 1;
        }
    }
    const uint64_t bound = flood_round_bound(cs);
    std::vector<size_t> perm(ntiles);
    for (size_t i = 0; i < ntiles; i++) perm[i] = order == 1 ? ntiles - 1 - i : i;
    uint64_t round = 0;
    for (bool marked = true; marked; round++) {
        if (round >= bound) return 6;
        marked = false;
        std::vector<uint8_t>&cur = act[round & 1], &next = act[(round + 1) & 1];
        if (order == 2) for (size_t i = ntiles; i > 1; i--) std::swap(perm[i - 1], perm[lcg(rng) % i]);
        if (order == 3) snap = reached;
        for (size_t k = 0; k < ntiles; k++) {
            const size_t ti = perm[k];
            if (!cur[ti]) continue;
            cur[ti] = 0;
            const uint32_t tx = (uint32_t)(ti % nt[0]), ty = (uint32_t)((ti / nt[0]) % nt[1]), tz = (uint32_t)(ti / ((size_t)nt[0] * nt[1]));
            uint32_t ext[VRT_FLOOD_EXT_ROWS];
            for (uint32_t e = 0; e < VRT_FLOOD_EXT_ROWS; e++) ext[e] = flood_ext_row(conn, (order == 3 ? snap : reached).data(), nt, tx, ty, tz, e);
            // (a tile's own rows are written by the tile alone, once a round: they are the same in both)
            flood_tile_relax(conn, &passable[ti * 64], ext);
            uint32_t wake = 0;
            for (uint32_t r = 0; r < 64; r++) {
                const uint32_t before = reached[ti * 64 + r], after = (ext[(r & 7) + 1 + 10 * ((r >> 3) + 1)] >> 1) & 0xFFu;
                wake |= flood_wake_mask(conn, before, after, r & 7, r >> 3);
                reached[ti * 64 + r] = (uint8_t)after;
            }
            for (uint32_t o = 0; o < 27; o++) {
                if (!((wake >> o) & 1u)) continue;
                const int nx = (int)tx + (int)(o % 3) - 1, ny = (int)ty + (int)((o / 3) % 3) - 1, nz = (int)tz + (int)(o / 9) - 1;
                if (nx < 0 || nx >= (int)nt[0] || ny < 0 || ny >= (int)nt[1] || nz < 0 || nz >= (int)nt[2]) continue;
                next[flood_tile_index((uint32_t)nx, (uint32_t)ny, (uint32_t)nz, nt)] = 1;
                marked = true;
            }
        }
    }
    int64_t region = 0, changed = 0, rmn[3] = {1 << 30, 1 << 30, 1 << 30}, rmx[3] = {-1, -1, -1}, mn[3] = {1 << 30, 1 << 30, 1 << 30}, mx[3] = {-1, -1, -1};
    const bool measure = (flags & VRT_FLOOD_FLAG_MEASURE) != 0u;
    for (uint32_t z = 0; z < cs[2]; z++) for (uint32_t y = 0; y < cs[1]; y++) for (uint32_t x = 0; x < cs[0]; x++) {
        if (!((reached[flood_mask_byte(x, y, z, nt)] >> flood_mask_bit(x)) & 1u)) continue;
        const int64_t v[3] = {clo[0] + (int64_t)x, clo[1] + (int64_t)y, clo[2] + (int64_t)z};
        region++;
        for (int a = 0; a < 3; a++) { rmn[a] = std::min(rmn[a], v[a]); rmx[a] = std::max(rmx[a], v[a]); }
        if (measure || at(x, y, z) == id) continue;
        at(x, y, z) = (uint8_t)id;
        changed++;
        for (int a = 0; a < 3; a++) { mn[a] = std::min(mn[a], v[a]); mx[a] = std::max(mx[a], v[a]); }
    }
    res[0] = region; res[7] = seed_id; res[8] = changed; res[15] = (int64_t)round;
    for (int a = 0; a < 3; a++) {
        if (region) { res[1 + a] = rmn[a]; res[4 + a] = rmx[a] - rmn[a] + 1; }
        if (changed) { res[9 + a] = mn[a]; res[12 + a] = mx[a] - mn[a] + 1; }
    }
    return 0;
}

extern "C" {

int flood_args_ok_c(int32_t match, int32_t conn, uint32_t flags, const uint32_t size[3]) { return flood_args_ok(match, conn, flags, size) ? 1 : 0; }
int flood_sides_ok_c(const uint32_t cs[3]) { return flood_sides_ok(cs) ? 1 : 0; }
int flood_seed_inside_c(const int32_t seed[3], const int32_t clo[3], const uint32_t cs[3]) { return flood_seed_inside(seed, clo, cs) ? 1 : 0; }
int flood_passes_c(int32_t match, uint32_t id, uint32_t seed_id) { return flood_passes(match, id, seed_id) ? 1 : 0; }
void flood_tiles_c(const uint32_t cs[3], uint32_t nt[3]) { flood_tiles(cs, nt); }
uint64_t flood_tile_index_c(uint32_t tx, uint32_t ty, uint32_t tz, const uint32_t nt[3]) { return flood_tile_index(tx, ty, tz, nt); }
uint64_t flood_mask_byte_c(uint32_t rx, uint32_t ry, uint32_t rz, const uint32_t nt[3]) { return flood_mask_byte(rx, ry, rz, nt); }
uint32_t flood_mask_bit_c(uint32_t rx) { return flood_mask_bit(rx); }
uint64_t flood_round_bound_c(const uint32_t cs[3]) { return flood_round_bound(cs); }
uint32_t flood_ext_row_c(int conn, const uint8_t* reached, const uint32_t nt[3], uint32_t tx, uint32_t ty, uint32_t tz, uint32_t e)
{
    return flood_ext_row(conn, reached, nt, tx, ty, tz, e);
}
int flood_tile_relax_c(int conn, const uint8_t passable[64], uint32_t ext[100]) { return flood_tile_relax(conn, passable, ext) ? 1 : 0; }
uint32_t flood_wake_mask_c(int conn, uint32_t before, uint32_t after, uint32_t y, uint32_t z) { return flood_wake_mask(conn, before, after, y, z); }

}
