// A program of its own for -fsanitize=address,undefined: csrc/vrt_morph.h's host code (through morph_host.cpp's driver of the tiled
// algorithm) on seeded random volumes, operations, connectivities, radii, border settings, and bounds at the int32 edges, each
// held against the closed form written here: a cell is in dil_r(X) iff some cell of X lies within distance r.  Host code only.
// Prints "<calls> calls, <voxels> voxels changed"; a mismatch or a sanitizer report ends it with a non-zero status.
//   morph_fuzz [seed] [rounds]
#include <cstdio>
#include <cstdlib>

#include "morph_host.cpp"

namespace {

uint32_t lcg(uint64_t& s) { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
struct Rng { uint64_t s; uint32_t next() { return lcg(s); } uint32_t below(uint32_t n) { return next() % n; } };

// a set over the window [-p, dim + p)^3 of the infinite grid; outside the window every cell is `fill`
struct Set {
    int32_t dim[3]; int p; bool fill; std::vector<uint8_t> v;
    bool get(int64_t x, int64_t y, int64_t z) const
    {
        if (x < -p || x >= dim[0] + p || y < -p || y >= dim[1] + p || z < -p || z >= dim[2] + p) return fill;
        return v[(size_t)((x + p) + ((y + p) + (z + p) * (int64_t)(dim[1] + 2 * p)) * (int64_t)(dim[0] + 2 * p))] != 0;
    }
};

// dil_r (erode: ero_r) by the definition: every cell of the window looks at its whole ball
Set apply(const Set& X, int conn, int r, bool erode)
{
    Set out = X;
    size_t i = 0;
    for (int64_t z = -X.p; z < X.dim[2] + X.p; z++) for (int64_t y = -X.p; y < X.dim[1] + X.p; y++) for (int64_t x = -X.p; x < X.dim[0] + X.p; x++, i++) {
        bool any = false, all = true;
        for (int dz = -r; dz <= r && !(erode ? !all : any); dz++) for (int dy = -r; dy <= r; dy++) for (int dx = -r; dx <= r; dx++) {
            const int d = conn == 6 ? abs(dx) + abs(dy) + abs(dz) : std::max(abs(dx), std::max(abs(dy), abs(dz)));
            if (d > r) continue;
            const bool g = X.get(x + dx, y + dy, z + dz);
            any = any || g; all = all && g;
        }
        out.v[i] = erode ? all : any;
    }
    return out;
}

}

int main(int argc, char** argv)
{
    Rng rng{argc > 1 ? strtoull(argv[1], nullptr, 10) : 1ull};
    const int rounds = argc > 2 ? atoi(argv[2]) : 100;
    long long calls = 0, total = 0;
    const int32_t edge[] = {INT32_MIN, INT32_MIN + 1, -1, 0, 1, INT32_MAX - 1, INT32_MAX};
    for (int k = 0; k < rounds; k++) {
        const int32_t dim[3] = {(int32_t)(1 + rng.below(k % 8 == 0 ? 70 : 12)), (int32_t)(1 + rng.below(10)), (int32_t)(1 + rng.below(10))};
        const int32_t op = (int32_t)rng.below(5), conn = rng.below(2) ? 6 : 26;
        const int32_t radius = k % 8 == 0 ? 1 + (int32_t)rng.below(2) : (int32_t)(1 + rng.below(rng.below(4) ? 3 : 8));
        const uint32_t flags = rng.below(2) ? VRT_MORPH_FLAG_BORDER_SOLID : 0u, id = 1u + rng.below(255), pct = 20u + rng.below(70);
        std::vector<uint8_t> vol((size_t)dim[0] * dim[1] * dim[2]);
        for (uint8_t& v : vol) v = rng.below(100) < pct ? (uint8_t)(1 + rng.below(3)) : 0;
        int32_t lo[3];
        uint32_t size[3];
        for (int a = 0; a < 3; a++) {
            lo[a] = rng.below(3) ? (int32_t)rng.below((uint32_t)dim[a] + 6u) - 5 : 0;
            size[a] = rng.below(3) ? 1u + rng.below((uint32_t)dim[a] + 8u) : (uint32_t)dim[a];
            if (rng.below(16) == 0) lo[a] = edge[rng.below(7)];
            if (rng.below(16) == 0) size[a] = rng.below(2) ? VRT_MORPH_MAX_SIZE : 1u;
        }
        // the definition on the window: the volume and 2r + 1 cells around it
        Set S{{dim[0], dim[1], dim[2]}, 2 * radius + 1, (flags & VRT_MORPH_FLAG_BORDER_SOLID) != 0u, {}};
        S.v.assign((size_t)(dim[0] + 2 * S.p) * (dim[1] + 2 * S.p) * (dim[2] + 2 * S.p), S.fill ? 1 : 0);
        for (int z = 0; z < dim[2]; z++) for (int y = 0; y < dim[1]; y++) for (int x = 0; x < dim[0]; x++)
            S.v[(size_t)((x + S.p) + ((y + S.p) + (z + S.p) * (int64_t)(dim[1] + 2 * S.p)) * (int64_t)(dim[0] + 2 * S.p))] = vol[(size_t)(x + (y + z * dim[1]) * dim[0])] != 0;
        Set R = S;
        if (op == VRT_MORPH_OP_DILATE) R = apply(S, conn, radius, false);
        else if (op == VRT_MORPH_OP_ERODE || op == VRT_MORPH_OP_HOLLOW) R = apply(S, conn, radius, true);
        else if (op == VRT_MORPH_OP_OPEN) R = apply(apply(S, conn, radius, true), conn, radius, false);
        else R = apply(apply(S, conn, radius, false), conn, radius, true);
        std::vector<uint8_t> want = vol;
        long long added = 0, removed = 0;
        for (int64_t z = 0; z < dim[2]; z++) for (int64_t y = 0; y < dim[1]; y++) for (int64_t x = 0; x < dim[0]; x++) {
            if (x < lo[0] || x >= (int64_t)lo[0] + size[0] || y < lo[1] || y >= (int64_t)lo[1] + size[1] || z < lo[2] || z >= (int64_t)lo[2] + size[2]) continue;
            uint8_t& v = want[(size_t)(x + (y + z * dim[1]) * dim[0])];
            const bool in = op == VRT_MORPH_OP_HOLLOW ? (v != 0 && !R.get(x, y, z)) : R.get(x, y, z);
            if (in && v == 0) { v = (uint8_t)id; added++; }
            else if (!in && v != 0) { v = 0; removed++; }
        }
        for (uint32_t measure = 0; measure < 2; measure++) {
            std::vector<uint8_t> got = vol;
            int64_t res[16];
            const int rc = morph_run_c(dim, got.data(), op, conn, radius, flags | (measure ? VRT_MORPH_FLAG_MEASURE : 0u), id, lo, size, res);
            const bool same = got == (measure ? vol : want);
            if (rc != 0 || res[0] != added || res[1] != removed || res[2] != (measure ? 0 : added + removed) || !same) {
                fprintf(stderr, "round %d op %d conn %d r %d flags %u measure %u: rc %d, added %lld (expected %lld), removed %lld (expected %lld), volumes %s\n", k, op, conn,
                        radius, flags, measure, rc, (long long)res[0], added, (long long)res[1], removed, same ? "equal" : "differ");
                return 1;
            }
            calls++;
        }
        if ((op == VRT_MORPH_OP_ERODE || op == VRT_MORPH_OP_OPEN || op == VRT_MORPH_OP_HOLLOW) && added) { fprintf(stderr, "round %d: op %d added a voxel\n", k, op); return 1; }
        if ((op == VRT_MORPH_OP_DILATE || op == VRT_MORPH_OP_CLOSE) && removed) { fprintf(stderr, "round %d: op %d removed a voxel\n", k, op); return 1; }
        total += added + removed;
    }
    printf("%lld calls, %lld voxels changed\n", calls, total);
    return 0;
}
