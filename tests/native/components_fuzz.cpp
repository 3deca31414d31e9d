// A program of its own for -fsanitize=address,undefined: csrc/vrt_components.h's host code (through components_host.cpp) on seeded
// random volumes, predicates, connectivities and bounds -- some at the int32 edges -- each held against a depth-first search
// written here over all 26 or 6 neighbours.  Host code only.
// Prints "<calls> calls, <components> components"; a mismatch or a sanitizer report ends it with a non-zero status.
//   components_fuzz [seed] [rounds]
#include <cstdio>
#include <cstdlib>

#include "components_host.cpp"

namespace {

uint32_t lcg(uint64_t& s) { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
struct Rng { uint64_t s; uint32_t next() { return lcg(s); } uint32_t below(uint32_t n) { return next() % n; } };

int fail_at(const char* what, uint32_t call) { printf("call %u: %s\n", call, what); return 1; }

} // namespace

int main(int argc, char** argv)
{
    Rng rng{argc > 1 ? strtoull(argv[1], nullptr, 10) : 1ull};
    const uint32_t rounds = argc > 2 ? (uint32_t)strtoul(argv[2], nullptr, 10) : 50u;
    uint64_t components = 0;
    for (uint32_t call = 0; call < rounds; call++) {
        const int32_t dim[3] = {(int32_t)(1u + rng.below(21u)), (int32_t)(1u + rng.below(19u)), (int32_t)(1u + rng.below(18u))};
        const uint32_t density = 1u + rng.below(9u);
        std::vector<uint8_t> vol((size_t)dim[0] * dim[1] * dim[2]);
        for (auto& v : vol) v = rng.below(10u) < density ? (uint8_t)(1u + rng.below(3u)) : 0;
        const int32_t match = (int32_t)rng.below(3u), conn = rng.below(2u) ? 26 : 6;
        int32_t lo[3];
        uint32_t size[3];
        for (int a = 0; a < 3; a++) {
            switch (rng.below(4u)) {
            case 0:  lo[a] = 0; size[a] = (uint32_t)dim[a]; break;
            case 1:  lo[a] = INT32_MIN; size[a] = 1u << 30; break;                    // wholly below the volume
            case 2:  lo[a] = -(int32_t)rng.below(5u); size[a] = 1u + rng.below(30u); break;
            default: lo[a] = INT32_MAX - (int32_t)rng.below(3u); size[a] = 1u << 30; break;  // lo + size beyond int32
            }
        }
        if (call % 3u == 0u) for (int a = 0; a < 3; a++) { lo[a] = -(int32_t)rng.below(3u); size[a] = (uint32_t)dim[a] + rng.below(4u); }
        int64_t res[9];
        std::vector<uint32_t> labels(vol.size());
        std::vector<CompRecord> rec(vol.size());
        if (comp_run_c(dim, vol.data(), match, conn, 0u, lo, size, rec.data(), rec.size(), labels.data(), res) != 0) return fail_at("refused", call);
        const uint32_t n = (uint32_t)res[0];
        if (n == 0u) continue;
        const int32_t clo[3] = {(int32_t)res[3], (int32_t)res[4], (int32_t)res[5]};
        const uint32_t cs[3] = {(uint32_t)res[6], (uint32_t)res[7], (uint32_t)res[8]};
        const size_t nv = (size_t)cs[0] * cs[1] * cs[2];
        auto id_at = [&](uint32_t x, uint32_t y, uint32_t z) { return vol[(size_t)(clo[0] + (int32_t)x) + ((size_t)(clo[1] + (int32_t)y) + (size_t)(clo[2] + (int32_t)z) * dim[1]) * dim[0]]; };
        // the search: ascending linear index, a stack, every neighbour of the connectivity
        std::vector<uint32_t> want(nv, VRT_COMP_NONE);
        uint32_t next = 0;
        uint64_t total = 0;
        for (size_t i = 0; i < nv; i++) {
            const uint32_t x0 = (uint32_t)(i % cs[0]), y0 = (uint32_t)((i / cs[0]) % cs[1]), z0 = (uint32_t)(i / ((size_t)cs[0] * cs[1]));
            const uint32_t k = comp_key(match, id_at(x0, y0, z0));
            if (k == 0u || want[i] != VRT_COMP_NONE) continue;
            std::vector<size_t> stack{i};
            want[i] = next;
            uint64_t count = 0;
            while (!stack.empty()) {
                const size_t c = stack.back();
                stack.pop_back();
                count++;
                const int64_t x = (int64_t)(c % cs[0]), y = (int64_t)((c / cs[0]) % cs[1]), z = (int64_t)(c / ((size_t)cs[0] * cs[1]));
                for (int dz = -1; dz <= 1; dz++) for (int dy = -1; dy <= 1; dy++) for (int dx = -1; dx <= 1; dx++) {
                    const int f = (dx != 0) + (dy != 0) + (dz != 0);
                    if (f == 0 || (conn == 6 && f != 1)) continue;
                    const int64_t px = x + dx, py = y + dy, pz = z + dz;
                    if (px < 0 || px >= (int64_t)cs[0] || py < 0 || py >= (int64_t)cs[1] || pz < 0 || pz >= (int64_t)cs[2]) continue;
                    const size_t m = (size_t)px + ((size_t)py + (size_t)pz * cs[1]) * cs[0];
                    if (want[m] != VRT_COMP_NONE || comp_key(match, id_at((uint32_t)px, (uint32_t)py, (uint32_t)pz)) != k) continue;
                    want[m] = next;
                    stack.push_back(m);
                }
            }
            if (next >= n) return fail_at("more components than reported", call);
            if (rec[next].voxels != count) return fail_at("a record's count", call);
            if (rec[next].root[0] != clo[0] + (int32_t)x0 || rec[next].root[1] != clo[1] + (int32_t)y0 || rec[next].root[2] != clo[2] + (int32_t)z0) return fail_at("a record's root", call);
            if (rec[next].id != id_at(x0, y0, z0)) return fail_at("a record's id", call);
            total += count;
            next++;
        }
        if (next != n || (uint64_t)res[1] != total) return fail_at("the component or voxel count", call);
        for (size_t i = 0; i < nv; i++)
            if (labels[i] != want[i]) return fail_at("a label", call);
        if (rec[(size_t)res[2]].voxels == 0) return fail_at("the largest", call);
        for (uint32_t k = 0; k < n; k++)
            if (rec[k].voxels > rec[(size_t)res[2]].voxels || (rec[k].voxels == rec[(size_t)res[2]].voxels && k < (uint32_t)res[2])) return fail_at("the largest", call);
        components += n;
    }
    printf("%u calls, %llu components\n", rounds, (unsigned long long)components);
    return 0;
}
