// Host build of csrc/vrt_edit.h for tests/test_scene_edit_cpu.py: the statements the scene-edit kernels rest on, checked
// against a brute-force rebuild.  edit_sweep() draws small volumes, boxes and caps, builds the eight open-coded clearance
// fields by brute force before and after the edit, and compares the rebuilt fields with the old ones updated the way
// launch_edit_fields does it: R_o recomputed by three clamped one-sided passes that read nothing outside E, the open cells of
// Q_o from AND scans seeded with the open state just beyond Q_o's far faces, the wall clearance for the re-closed cells of
// Q_o outside R_o, everything else untouched.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../voxel-raytracing_amd/csrc/vrt_edit.h"

using namespace vrt;

namespace {

struct Vol {
    int W, H, D;
    std::vector<uint8_t> v;
    bool inside(int x, int y, int z) const { return x >= 0 && y >= 0 && z >= 0 && x < W && y < H && z < D; }
    size_t at(int x, int y, int z) const { return (size_t)x + ((size_t)y + (size_t)z * H) * W; }
    bool solid(int x, int y, int z) const { return !inside(x, y, z) || v[at(x, y, z)] != 0; }   // outside counts as solid
};

// the definition: side of the largest empty cube cornered at p towards s, capped; open: nothing solid in the corner box
void brute(const Vol& V, int cap, int o, std::vector<uint8_t>& coded, std::vector<uint8_t>& open)
{
    const int s[3] = {(o & 1) ? 1 : -1, (o & 2) ? 1 : -1, (o & 4) ? 1 : -1};
    coded.assign(V.v.size(), 0); open.assign(V.v.size(), 0);
    for (int z = 0; z < V.D; z++) for (int y = 0; y < V.H; y++) for (int x = 0; x < V.W; x++) {
        if (V.v[V.at(x, y, z)]) continue;
        int k = 0;
        for (; k < cap; k++) {                                  // can the cube grow to side k + 1?
            bool hit = false;
            for (int c = 0; c <= k && !hit; c++) for (int b = 0; b <= k && !hit; b++) for (int a = 0; a <= k && !hit; a++)
                if ((a == k || b == k || c == k) && V.solid(x + a * s[0], y + b * s[1], z + c * s[2])) hit = true;
            if (hit) break;
        }
        bool op = true;
        for (int zz = z; zz >= 0 && zz < V.D && op; zz += s[2]) for (int yy = y; yy >= 0 && yy < V.H && op; yy += s[1])
            for (int xx = x; xx >= 0 && xx < V.W && op; xx += s[0]) if (V.v[V.at(xx, yy, zz)]) op = false;
        open[V.at(x, y, z)] = op;
        coded[V.at(x, y, z)] = op ? 0 : (uint8_t)k;
    }
}

// one clamped one-sided pass at position p of a line of n values; out of the line is solid
int pass_at(const std::vector<int>& line, int p, int dir, int cap)
{
    int best = line[p];
    for (int t = 1; t < best; t++) {
        const int q = p + t * dir;
        const int val = (q < 0 || q >= (int)line.size()) ? 0 : line[q];
        const int m = val > t ? val : t;
        best = best < m ? best : m;
    }
    return best < cap ? best : cap;
}

// the octant's field `f` (open-coded, as before the edit) brought up to date for the volume V (after the edit) and the box
void update(const Vol& V, int cap, int o, const int lo[3], const int hi[3], std::vector<uint8_t>& f)
{
    const int dim[3] = {V.W, V.H, V.D};
    const int s[3] = {(o & 1) ? 1 : -1, (o & 2) ? 1 : -1, (o & 4) ? 1 : -1};
    EditSpan R[3], E[3], Q[3];
    for (int a = 0; a < 3; a++) { R[a] = edit_span_r(lo[a], hi[a], dim[a], s[a], cap); E[a] = edit_span_e(lo[a], hi[a], dim[a], cap); Q[a] = edit_span_q(lo[a], hi[a], dim[a], s[a]); }
    const int ex = E[0].hi - E[0].lo, ey = E[1].hi - E[1].lo, ez = E[2].hi - E[2].lo;
    auto ei = [&](int x, int y, int z) { return (size_t)(x - E[0].lo) + ((size_t)(y - E[1].lo) + (size_t)(z - E[2].lo) * ey) * ex; };
    // pass x: R_x x E_y x E_z, reading voxels of E only
    std::vector<int> A((size_t)ex * ey * ez, -1), B(A.size(), -1), Cc(A.size(), -1);
    for (int z = E[2].lo; z < E[2].hi; z++) for (int y = E[1].lo; y < E[1].hi; y++) {
        std::vector<int> line(ex);
        for (int x = E[0].lo; x < E[0].hi; x++) line[x - E[0].lo] = V.v[V.at(x, y, z)] ? 0 : cap;
        for (int x = R[0].lo; x < R[0].hi; x++) A[ei(x, y, z)] = pass_at(line, x - E[0].lo, s[0], cap);
    }
    for (int z = E[2].lo; z < E[2].hi; z++) for (int x = R[0].lo; x < R[0].hi; x++) {
        std::vector<int> line(ey);
        for (int y = E[1].lo; y < E[1].hi; y++) line[y - E[1].lo] = A[ei(x, y, z)];
        for (int y = R[1].lo; y < R[1].hi; y++) B[ei(x, y, z)] = pass_at(line, y - E[1].lo, s[1], cap);
    }
    for (int y = R[1].lo; y < R[1].hi; y++) for (int x = R[0].lo; x < R[0].hi; x++) {
        std::vector<int> line(ez);
        for (int z = E[2].lo; z < E[2].hi; z++) line[z - E[2].lo] = B[ei(x, y, z)];
        for (int z = R[2].lo; z < R[2].hi; z++) f[V.at(x, y, z)] = (uint8_t)pass_at(line, z - E[2].lo, s[2], cap);
    }
    // open cells of Q_o: scans along y, z, x, each seeded with the open state -- read from the field -- just beyond the far face
    auto open_before = [&](int x, int y, int z) { return !V.inside(x, y, z) || (f[V.at(x, y, z)] == 0 && V.v[V.at(x, y, z)] == 0); };
    const int qx = Q[0].hi - Q[0].lo, qy = Q[1].hi - Q[1].lo, qz = Q[2].hi - Q[2].lo;
    auto qi = [&](int x, int y, int z) { return (size_t)(x - Q[0].lo) + ((size_t)(y - Q[1].lo) + (size_t)(z - Q[2].lo) * qy) * qx; };
    std::vector<uint8_t> T0((size_t)qx * qy * qz), T1(T0.size()), T2(T0.size());
    auto far_to_near = [](int lo_, int n, int dir, int t) { return dir > 0 ? lo_ + n - 1 - t : lo_ + t; };
    for (int z = Q[2].lo; z < Q[2].hi; z++) for (int x = Q[0].lo; x < Q[0].hi; x++) {
        bool flag = open_before(x, s[1] > 0 ? Q[1].hi : Q[1].lo - 1, z);
        for (int t = 0; t < qy; t++) { const int y = far_to_near(Q[1].lo, qy, s[1], t); flag = flag && V.v[V.at(x, y, z)] == 0; T0[qi(x, y, z)] = flag; }
    }
    for (int y = Q[1].lo; y < Q[1].hi; y++) for (int x = Q[0].lo; x < Q[0].hi; x++) {
        bool flag = open_before(x, y, s[2] > 0 ? Q[2].hi : Q[2].lo - 1);
        for (int t = 0; t < qz; t++) { const int z = far_to_near(Q[2].lo, qz, s[2], t); flag = flag && T0[qi(x, y, z)]; T1[qi(x, y, z)] = flag; }
    }
    for (int z = Q[2].lo; z < Q[2].hi; z++) for (int y = Q[1].lo; y < Q[1].hi; y++) {
        bool flag = open_before(s[0] > 0 ? Q[0].hi : Q[0].lo - 1, y, z);
        for (int t = 0; t < qx; t++) { const int x = far_to_near(Q[0].lo, qx, s[0], t); flag = flag && T1[qi(x, y, z)]; T2[qi(x, y, z)] = flag; }
    }
    for (int z = Q[2].lo; z < Q[2].hi; z++) for (int y = Q[1].lo; y < Q[1].hi; y++) for (int x = Q[0].lo; x < Q[0].hi; x++) {
        uint8_t& cell = f[V.at(x, y, z)];
        if (T2[qi(x, y, z)]) { cell = 0; continue; }
        const bool in_r = x >= R[0].lo && x < R[0].hi && y >= R[1].lo && y < R[1].hi && z >= R[2].lo && z < R[2].hi;
        if (in_r) continue;
        if (cell == 0 && V.v[V.at(x, y, z)] == 0) cell = (uint8_t)edit_wall_clearance(x, y, z, V.W, V.H, V.D, s[0], s[1], s[2], cap);
    }
}

} // namespace

extern "C" {

// out[0] = edits checked, out[1] = octant fields that differ from the rebuild, out[2] = bytes changed outside Q_o,
// out[3] = edits of each kind seen, as bits (1 random, 2 wall / corner, 4 wider than the cap, 8 whole volume, 16 one voxel)
void edit_sweep(uint32_t seed, int trials, uint64_t out[4])
{
    std::mt19937 rng(seed);
    auto ri = [&](int a, int b) { return a + (int)(rng() % (uint32_t)(b - a + 1)); };     // [a, b]
    out[0] = out[1] = out[2] = out[3] = 0;
    for (int trial = 0; trial < trials; trial++) {
        Vol V;
        V.W = ri(3, 10); V.H = ri(3, 10); V.D = ri(3, 10);
        const int cap = ri(2, 5);
        const int dens = ri(0, 2);                              // empty, sparse, denser
        V.v.resize((size_t)V.W * V.H * V.D);
        for (auto& b : V.v) b = (dens && (int)(rng() % 100) < (dens == 1 ? 2 : 10)) ? (uint8_t)ri(1, 8) : 0;
        const int dim[3] = {V.W, V.H, V.D};
        int lo[3], hi[3];
        const int kind = trial % 5;
        for (int a = 0; a < 3; a++) {
            if (kind == 0) { lo[a] = ri(0, dim[a] - 1); hi[a] = ri(lo[a] + 1, dim[a]); }
            else if (kind == 1) { const int n = ri(1, dim[a]); lo[a] = (rng() & 1) ? 0 : dim[a] - n; hi[a] = lo[a] + n; }     // at a wall on every axis: a corner
            else if (kind == 2) { const int n = dim[a] > cap ? ri(cap + 1, dim[a]) : dim[a]; lo[a] = ri(0, dim[a] - n); hi[a] = lo[a] + n; }
            else if (kind == 3) { lo[a] = 0; hi[a] = dim[a]; }
            else { lo[a] = ri(0, dim[a] - 1); hi[a] = lo[a] + 1; }
        }
        out[3] |= 1u << kind;
        Vol N = V;
        const int fill = ri(0, 2);                              // carve, mixed, fill
        for (int z = lo[2]; z < hi[2]; z++) for (int y = lo[1]; y < hi[1]; y++) for (int x = lo[0]; x < hi[0]; x++)
            N.v[N.at(x, y, z)] = fill == 0 ? 0 : (fill == 2 || rng() % 100 < 30) ? (uint8_t)ri(1, 8) : 0;
        out[0]++;
        for (int o = 0; o < 8; o++) {
            std::vector<uint8_t> f0, f1, op;
            brute(V, cap, o, f0, op);
            brute(N, cap, o, f1, op);
            EditSpan Q[3];
            for (int a = 0; a < 3; a++) Q[a] = edit_span_q(lo[a], hi[a], dim[a], ((o >> a) & 1) ? 1 : -1);
            for (int z = 0; z < V.D; z++) for (int y = 0; y < V.H; y++) for (int x = 0; x < V.W; x++) {
                const bool in_q = x >= Q[0].lo && x < Q[0].hi && y >= Q[1].lo && y < Q[1].hi && z >= Q[2].lo && z < Q[2].hi;
                if (!in_q && f0[V.at(x, y, z)] != f1[V.at(x, y, z)]) out[2]++;
            }
            update(N, cap, o, lo, hi, f0);
            if (f0 != f1) out[1]++;
        }
    }
}

int edit_in_place_c(int W, int H, int D, const int lo[3], const int hi[3]) { return edit_in_place(W, H, D, lo, hi, VRT_EDIT_CAP) ? 1 : 0; }

}
