// A program of its own for -fsanitize=address,undefined: csrc/vrt_flood.h's host code (through flood_host.cpp's driver of the tiled
// algorithm) on seeded random volumes, predicates, connectivities, tile orders, and bounds and seeds at the int32 edges, each
// held against a queue of voxels written here.  Prints "<floods> floods, <voxels> voxels reached"; a mismatch or a sanitizer
// report ends it with a non-zero status.
//   flood_fuzz [seed] [rounds]
#include <cstdio>
#include <cstdlib>
#include <array>
#include <deque>

#include "flood_host.cpp"

namespace {

struct Rng { uint64_t s; uint32_t next() { return lcg(s); } uint32_t below(uint32_t n) { return next() % n; } };

// the definition: the seed's component among the passing voxels of the clipped bounds; -> voxels reached, vol rewritten
int64_t plain(const int32_t dim[3], std::vector<uint8_t>& vol, const int32_t seed[3], const int32_t lo[3], const uint32_t size[3], int32_t match, int32_t conn, uint32_t id)
{
    int64_t l[3], h[3];
    for (int a = 0; a < 3; a++) {
        l[a] = lo[a] > 0 ? lo[a] : 0;
        h[a] = (int64_t)lo[a] + size[a] < dim[a] ? (int64_t)lo[a] + size[a] : dim[a];
        if (h[a] <= l[a] || seed[a] < l[a] || seed[a] >= h[a]) return 0;
    }
    auto at = [&](int64_t x, int64_t y, int64_t z) -> uint8_t& { return vol[(size_t)(x + (y + z * dim[1]) * dim[0])]; };
    const uint32_t seed_id = at(seed[0], seed[1], seed[2]);
    if (!(match == VRT_FLOOD_MATCH_SAME || seed_id != 0u)) return 0;
    std::vector<uint8_t> got(vol.size(), 0);
    std::deque<std::array<int64_t, 3>> queue;
    got[(size_t)(seed[0] + ((int64_t)seed[1] + (int64_t)seed[2] * dim[1]) * dim[0])] = 1;
    queue.push_back({seed[0], seed[1], seed[2]});
    int64_t n = 0;
    while (!queue.empty()) {
        const std::array<int64_t, 3> v = queue.front();
        queue.pop_front();
        n++;
        for (int dz = -1; dz <= 1; dz++) for (int dy = -1; dy <= 1; dy++) for (int dx = -1; dx <= 1; dx++) {
            const int faces = (dx != 0) + (dy != 0) + (dz != 0);
            if (faces == 0 || (conn == 6 && faces != 1)) continue;
            const int64_t w[3] = {v[0] + dx, v[1] + dy, v[2] + dz};
            if (w[0] < l[0] || w[0] >= h[0] || w[1] < l[1] || w[1] >= h[1] || w[2] < l[2] || w[2] >= h[2]) continue;
            uint8_t& g = got[(size_t)(w[0] + (w[1] + w[2] * dim[1]) * dim[0])];
            const uint32_t vid = at(w[0], w[1], w[2]);
            if (g || !(match == VRT_FLOOD_MATCH_SAME ? vid == seed_id : vid != 0u)) continue;
            g = 1;
            queue.push_back({w[0], w[1], w[2]});
        }
    }
    for (size_t i = 0; i < vol.size(); i++)
        if (got[i]) vol[i] = (uint8_t)id;
    return n;
}

}

int main(int argc, char** argv)
{
    Rng rng{argc > 1 ? strtoull(argv[1], nullptr, 10) : 1ull};
    const int rounds = argc > 2 ? atoi(argv[2]) : 200;
    long long floods = 0, reached = 0;
    const int32_t edge[] = {INT32_MIN, INT32_MIN + 1, -1, 0, 1, INT32_MAX - 1, INT32_MAX};
    for (int r = 0; r < rounds; r++) {
        const int32_t dim[3] = {(int32_t)(1 + rng.below(40)), (int32_t)(1 + rng.below(20)), (int32_t)(1 + rng.below(20))};
        const int32_t conn = rng.below(2) ? 6 : 26, match = (int32_t)rng.below(2);
        const uint32_t pct = conn == 6 ? 31u : 10u, id = rng.below(4) ? rng.below(256) : 0u;
        std::vector<uint8_t> vol((size_t)dim[0] * dim[1] * dim[2]);
        for (uint8_t& v : vol) v = rng.below(100) < pct ? (uint8_t)(1 + rng.below(3)) : 0;
        int32_t seed[3], lo[3];
        uint32_t size[3];
        for (int a = 0; a < 3; a++) {
            seed[a] = (int32_t)rng.below((uint32_t)dim[a]);
            lo[a] = rng.below(3) ? (int32_t)rng.below((uint32_t)dim[a] + 6u) - 5 : 0;
            size[a] = rng.below(3) ? 1u + rng.below((uint32_t)dim[a] + 8u) : (uint32_t)dim[a];
            if (rng.below(16) == 0) lo[a] = edge[rng.below(7)];
            if (rng.below(16) == 0) size[a] = rng.below(2) ? VRT_FLOOD_MAX_SIZE : 1u;
            if (rng.below(16) == 0) seed[a] = edge[rng.below(7)];
        }
        std::vector<uint8_t> want = vol;
        int64_t l[3], h[3];
        int32_t clo[3];
        uint32_t cs[3];
        for (int a = 0; a < 3; a++) { l[a] = lo[a]; h[a] = (int64_t)lo[a] + size[a]; }
        const bool inside = brush_clip(l, h, dim, clo, cs) && flood_seed_inside(seed, clo, cs);
        const int64_t n = inside ? plain(dim, want, seed, lo, size, match, conn, id) : 0;
        for (int order = 0; order < 4; order++) {
            std::vector<uint8_t> got = vol;
            int64_t res[16];
            const int rc = flood_run_c(dim, got.data(), seed, lo, size, match, conn, 0u, id, order, rng.s, res);
            if (rc != 0 || res[0] != n || got != want) {
                fprintf(stderr, "round %d order %d: rc %d, region %lld, expected %lld, volumes %s\n", r, order, rc, (long long)res[0], (long long)n, got == want ? "equal" : "differ");
                return 1;
            }
            if ((uint64_t)res[15] > flood_round_bound(cs) && inside) { fprintf(stderr, "round %d: %lld rounds\n", r, (long long)res[15]); return 1; }
            floods++;
        }
        reached += n;
    }
    printf("%lld floods, %lld voxels reached\n", floods, reached);
    return 0;
}
