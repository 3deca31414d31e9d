// Host build of csrc/vrt_brick_edit.h for tests/test_brick_edit_cpu.py: the statements the brick-scene edits rest on, checked
// against a brute-force build.  brick_edit_sweep() draws brick lattices, voxel contents and boxes, builds by the definitions
// (vrt_march_brick.h brick_clear, VolumeView::bcoarse / bfine / bentry; k_brick_fine) the occupancy, the per-voxel clearances of the occupied
// bricks, the eight coarse fields with their open bits and the packed entries before and after the edit, and checks that
//   * the fine bytes of every brick outside F are the same, and the ids and the occupancy of every brick outside T;
//   * an edit that changes no brick's occupancy changes no coarse byte, no open bit and no entry;
//   * otherwise a coarse clearance changes only inside R_o, an open bit only inside Q_o;
//   * the old coarse fields updated the way launch_bedit_coarse does it -- R_o from a transform of the sub-lattice E alone (its
//     outside solid), the open bits of Q_o from AND scans seeded with the old bits just beyond Q_o's far faces -- equal the new.
#include <cstdint>
#include <cstring>
#include <random>
#include <vector>

#include "../../voxel-raytracing_amd/csrc/vrt_brick_edit.h"

using namespace vrt;

namespace {

const int CAP = VRT_BRICK_EDIT_CAP;

struct Scene {
    int nb[3];
    std::vector<uint8_t> vox;                                  // 8 nbx x 8 nby x 8 nbz, x fastest
    int W() const { return nb[0] * 8; }
    int H() const { return nb[1] * 8; }
    int D() const { return nb[2] * 8; }
    size_t nbricks() const { return (size_t)nb[0] * nb[1] * nb[2]; }
    size_t bi(int x, int y, int z) const { return (size_t)x + ((size_t)y + (size_t)z * nb[1]) * nb[0]; }
    bool in_vol(int x, int y, int z) const { return x >= 0 && y >= 0 && z >= 0 && x < W() && y < H() && z < D(); }
    bool solid(int x, int y, int z) const { return !in_vol(x, y, z) || vox[(size_t)x + ((size_t)y + (size_t)z * H()) * W()] != 0; }
};

struct Built {
    std::vector<uint8_t> occ;                                  // per brick
    std::vector<uint8_t> fine;                                 // per brick 8 x 512 (zeros for an empty brick)
    std::vector<uint8_t> coarse[8];                            // per brick: low 7 bits clearance in bricks, bit 7 open
    std::vector<uint64_t> entry;                               // brick_entry_pack's layout, the pointer field: 0 empty, 1 occupied
};

bool in_lattice(const Scene& S, int x, int y, int z) { return x >= 0 && y >= 0 && z >= 0 && x < S.nb[0] && y < S.nb[1] && z < S.nb[2]; }

void build(const Scene& S, bool with_fine, Built& B)
{
    const size_t n = S.nbricks();
    B.occ.assign(n, 0);
    for (int z = 0; z < S.D(); z++) for (int y = 0; y < S.H(); y++) for (int x = 0; x < S.W(); x++)
        if (S.vox[(size_t)x + ((size_t)y + (size_t)z * S.H()) * S.W()]) B.occ[S.bi(x >> 3, y >> 3, z >> 3)] = 1;
    auto bsolid = [&](int x, int y, int z) { return !in_lattice(S, x, y, z) || B.occ[S.bi(x, y, z)] != 0; };
    for (int o = 0; o < 8; o++) {
        const int s[3] = {(o & 1) ? 1 : -1, (o & 2) ? 1 : -1, (o & 4) ? 1 : -1};
        B.coarse[o].assign(n, 0);
        for (int z = 0; z < S.nb[2]; z++) for (int y = 0; y < S.nb[1]; y++) for (int x = 0; x < S.nb[0]; x++) {
            if (B.occ[S.bi(x, y, z)]) continue;
            int k = 0;
            for (; k < CAP; k++) {                              // can the cube of empty bricks grow to side k + 1?
                bool hit = false;
                for (int c = 0; c <= k && !hit; c++) for (int b = 0; b <= k && !hit; b++) for (int a = 0; a <= k && !hit; a++)
                    if ((a == k || b == k || c == k) && bsolid(x + a * s[0], y + b * s[1], z + c * s[2])) hit = true;
                if (hit) break;
            }
            bool open = true;
            for (int zz = z; zz >= 0 && zz < S.nb[2] && open; zz += s[2]) for (int yy = y; yy >= 0 && yy < S.nb[1] && open; yy += s[1])
                for (int xx = x; xx >= 0 && xx < S.nb[0] && open; xx += s[0]) if (B.occ[S.bi(xx, yy, zz)]) open = false;
            B.coarse[o][S.bi(x, y, z)] = (uint8_t)(k | (open ? 0x80 : 0));
        }
    }
    B.entry.assign(n, 0);
    for (size_t i = 0; i < n; i++) {
        uint32_t lo = B.occ[i] ? 1u : 0u, hi = 0;
        for (int o = 0; o < 8; o++) {
            const uint32_t c = B.coarse[o][i] & 0x7Fu;
            hi |= (c > 15u ? 15u : c) << (4 * o);
            if (B.coarse[o][i] & 0x80u) lo |= 1u << (24 + o);
        }
        B.entry[i] = (uint64_t)lo | ((uint64_t)hi << 32);
    }
    B.fine.assign(with_fine ? n * 4096 : 0, 0);
    if (!with_fine) return;
    // per voxel of an occupied brick: the largest empty cube of voxels cornered there, looking no further than the brick's 26
    // neighbours (beyond them, and outside the volume, counts as solid), capped at 16
    for (int bz = 0; bz < S.nb[2]; bz++) for (int by = 0; by < S.nb[1]; by++) for (int bx = 0; bx < S.nb[0]; bx++) {
        const size_t b = S.bi(bx, by, bz);
        if (!B.occ[b]) continue;
        const int w0[3] = {bx * 8 - 8, by * 8 - 8, bz * 8 - 8};
        auto wsolid = [&](int x, int y, int z) {
            if (x < w0[0] || y < w0[1] || z < w0[2] || x >= w0[0] + 24 || y >= w0[1] + 24 || z >= w0[2] + 24) return true;
            return S.solid(x, y, z);
        };
        for (int o = 0; o < 8; o++) {
            const int s[3] = {(o & 1) ? 1 : -1, (o & 2) ? 1 : -1, (o & 4) ? 1 : -1};
            for (int v = 0; v < 512; v++) {
                const int x = bx * 8 + (v & 7), y = by * 8 + ((v >> 3) & 7), z = bz * 8 + (v >> 6);
                int k = 0;
                if (!S.solid(x, y, z))
                    for (; k < 16; k++) {
                        bool hit = false;
                        for (int c = 0; c <= k && !hit; c++) for (int bb = 0; bb <= k && !hit; bb++) for (int a = 0; a <= k && !hit; a++)
                            if ((a == k || bb == k || c == k) && wsolid(x + a * s[0], y + bb * s[1], z + c * s[2])) hit = true;
                        if (hit) break;
                    }
                B.fine[(b * 8 + (size_t)o) * 512 + (size_t)v] = (uint8_t)k;
            }
        }
    }
}

int pass_at(const std::vector<int>& line, int p, int dir)
{
    int best = line[p];
    for (int t = 1; t < best; t++) {
        const int q = p + t * dir;
        const int val = (q < 0 || q >= (int)line.size()) ? 0 : line[q];
        const int m = val > t ? val : t;
        best = best < m ? best : m;
    }
    return best < CAP ? best : CAP;
}

// the octant's coarse field f (as before the edit) brought up to date for the occupancy `occ` (after it), as launch_bedit_coarse does
void update_coarse(const Scene& S, const std::vector<uint8_t>& occ, int o, const EditSpan T[3], std::vector<uint8_t>& f)
{
    const int s[3] = {(o & 1) ? 1 : -1, (o & 2) ? 1 : -1, (o & 4) ? 1 : -1};
    EditSpan R[3], E[3], Q[3];
    for (int a = 0; a < 3; a++) { R[a] = brick_span_r(T[a], S.nb[a], s[a]); E[a] = brick_span_e(T[a], S.nb[a]); Q[a] = brick_span_q(T[a], S.nb[a], s[a]); }
    // the transform of the sub-lattice E, out of E = solid, over ALL of E (k_df_pass on the extracted lattice)
    const int en[3] = {E[0].hi - E[0].lo, E[1].hi - E[1].lo, E[2].hi - E[2].lo};
    auto ei = [&](int x, int y, int z) { return (size_t)x + ((size_t)y + (size_t)z * en[1]) * en[0]; };
    std::vector<int> A((size_t)en[0] * en[1] * en[2]), Bv(A.size()), Cv(A.size());
    for (int z = 0; z < en[2]; z++) for (int y = 0; y < en[1]; y++) for (int x = 0; x < en[0]; x++)
        A[ei(x, y, z)] = occ[S.bi(E[0].lo + x, E[1].lo + y, E[2].lo + z)] ? 0 : CAP + 1;
    for (int z = 0; z < en[2]; z++) for (int y = 0; y < en[1]; y++) {
        std::vector<int> line(en[0]);
        for (int x = 0; x < en[0]; x++) line[x] = A[ei(x, y, z)];
        for (int x = 0; x < en[0]; x++) { int best = line[x]; for (int t = 1; t < best; t++) { const int q = x + t * s[0]; const int val = (q < 0 || q >= en[0]) ? 0 : line[q]; const int m = val > t ? val : t; best = best < m ? best : m; } Bv[ei(x, y, z)] = best; }
    }
    for (int z = 0; z < en[2]; z++) for (int x = 0; x < en[0]; x++) {
        std::vector<int> line(en[1]);
        for (int y = 0; y < en[1]; y++) line[y] = Bv[ei(x, y, z)];
        for (int y = 0; y < en[1]; y++) { int best = line[y]; for (int t = 1; t < best; t++) { const int q = y + t * s[1]; const int val = (q < 0 || q >= en[1]) ? 0 : line[q]; const int m = val > t ? val : t; best = best < m ? best : m; } Cv[ei(x, y, z)] = best; }
    }
    for (int y = 0; y < en[1]; y++) for (int x = 0; x < en[0]; x++) {
        std::vector<int> line(en[2]);
        for (int z = 0; z < en[2]; z++) line[z] = Cv[ei(x, y, z)];
        for (int z = 0; z < en[2]; z++) {
            const int gx = E[0].lo + x, gy = E[1].lo + y, gz = E[2].lo + z;
            if (gx < R[0].lo || gx >= R[0].hi || gy < R[1].lo || gy >= R[1].hi || gz < R[2].lo || gz >= R[2].hi) continue;
            f[S.bi(gx, gy, gz)] = (uint8_t)pass_at(line, z, s[2]);             // k_bedit_copy: the open bit cleared
        }
    }
    // open bits of Q_o
    auto open_before = [&](int x, int y, int z) { return !in_lattice(S, x, y, z) || (f[S.bi(x, y, z)] & 0x80) != 0; };
    const int qn[3] = {Q[0].hi - Q[0].lo, Q[1].hi - Q[1].lo, Q[2].hi - Q[2].lo};
    auto qi = [&](int x, int y, int z) { return (size_t)(x - Q[0].lo) + ((size_t)(y - Q[1].lo) + (size_t)(z - Q[2].lo) * qn[1]) * qn[0]; };
    std::vector<uint8_t> T0((size_t)qn[0] * qn[1] * qn[2]), T1(T0.size()), T2(T0.size());
    auto far_to_near = [](int lo_, int n, int dir, int t) { return dir > 0 ? lo_ + n - 1 - t : lo_ + t; };
    for (int z = Q[2].lo; z < Q[2].hi; z++) for (int x = Q[0].lo; x < Q[0].hi; x++) {
        bool flag = open_before(x, s[1] > 0 ? Q[1].hi : Q[1].lo - 1, z);
        for (int t = 0; t < qn[1]; t++) { const int y = far_to_near(Q[1].lo, qn[1], s[1], t); flag = flag && !occ[S.bi(x, y, z)]; T0[qi(x, y, z)] = flag; }
    }
    for (int y = Q[1].lo; y < Q[1].hi; y++) for (int x = Q[0].lo; x < Q[0].hi; x++) {
        bool flag = open_before(x, y, s[2] > 0 ? Q[2].hi : Q[2].lo - 1);
        for (int t = 0; t < qn[2]; t++) { const int z = far_to_near(Q[2].lo, qn[2], s[2], t); flag = flag && T0[qi(x, y, z)]; T1[qi(x, y, z)] = flag; }
    }
    for (int z = Q[2].lo; z < Q[2].hi; z++) for (int y = Q[1].lo; y < Q[1].hi; y++) {
        bool flag = open_before(s[0] > 0 ? Q[0].hi : Q[0].lo - 1, y, z);
        for (int t = 0; t < qn[0]; t++) { const int x = far_to_near(Q[0].lo, qn[0], s[0], t); flag = flag && T1[qi(x, y, z)]; T2[qi(x, y, z)] = flag; }
    }
    for (int z = Q[2].lo; z < Q[2].hi; z++) for (int y = Q[1].lo; y < Q[1].hi; y++) for (int x = Q[0].lo; x < Q[0].hi; x++) {
        uint8_t& cell = f[S.bi(x, y, z)];
        cell = T2[qi(x, y, z)] ? (uint8_t)(cell | 0x80) : (uint8_t)(cell & 0x7F);
    }
}

bool inside(const EditSpan s[3], int x, int y, int z) { return x >= s[0].lo && x < s[0].hi && y >= s[1].lo && y < s[1].hi && z >= s[2].lo && z < s[2].hi; }

} // namespace

extern "C" {

// out[0] trials, [1] fine bytes changed outside F, [2] bricks outside T whose occupancy changed, [3] coarse clearances changed
// outside R_o, [4] open bits changed outside Q_o, [5] entries changed outside the union of the Q_o, [6] coarse bytes / entries
// changed by edits that changed no occupancy, [7] octant fields where the in-place update differs from the build, [8] edits that
// changed some occupancy, [9] of those, edits the rule sends to the full build, [10] trials with fine bytes, [11] kinds of box
// seen, as bits, [12] edits that emptied a brick, [13] edits that created one
void brick_edit_sweep(uint32_t seed, int trials, uint64_t out[14])
{
    std::mt19937 rng(seed);
    auto ri = [&](int a, int b) { return a + (int)(rng() % (uint32_t)(b - a + 1)); };
    memset(out, 0, 14 * sizeof(uint64_t));
    for (int trial = 0; trial < trials; trial++) {
        Scene S;
        const bool with_fine = trial % 2 == 0;
        if (with_fine) { S.nb[0] = ri(1, 4); S.nb[1] = ri(1, 3); S.nb[2] = ri(1, 3); }
        else {                                                  // long enough for the cap of 16 bricks to matter, on a random axis
            const int a = ri(0, 2);
            S.nb[a] = ri(18, 44); S.nb[(a + 1) % 3] = ri(1, 4); S.nb[(a + 2) % 3] = ri(1, 3);
        }
        S.vox.assign((size_t)S.W() * S.H() * S.D(), 0);
        const int pct = with_fine ? ri(0, 70) : ri(0, 40);     // share of occupied bricks
        for (int bz = 0; bz < S.nb[2]; bz++) for (int by = 0; by < S.nb[1]; by++) for (int bx = 0; bx < S.nb[0]; bx++) {
            if ((int)(rng() % 100) >= pct) continue;
            const int dens = ri(1, 100);
            bool any = false;
            for (int v = 0; v < 512; v++) {
                const bool set = (int)(rng() % 100) < dens;
                any = any || set;
                if (set) S.vox[(size_t)(bx * 8 + (v & 7)) + ((size_t)(by * 8 + ((v >> 3) & 7)) + (size_t)(bz * 8 + (v >> 6)) * S.H()) * S.W()] = (uint8_t)ri(1, 255);
            }
            if (!any) S.vox[(size_t)(bx * 8) + ((size_t)(by * 8) + (size_t)(bz * 8) * S.H()) * S.W()] = 1;
        }
        const int dim[3] = {S.W(), S.H(), S.D()};
        int lo[3], hi[3];
        const int kind = trial % 6;
        for (int a = 0; a < 3; a++) {
            if (kind == 0) { lo[a] = ri(0, dim[a] - 1); hi[a] = ri(lo[a] + 1, dim[a] < lo[a] + 20 ? dim[a] : lo[a] + 20); }
            else if (kind == 1) { const int b0 = ri(0, S.nb[a] - 1), b1 = ri(b0 + 1, S.nb[a] < b0 + 3 ? S.nb[a] : b0 + 3); lo[a] = b0 * 8; hi[a] = b1 * 8; }   // brick-aligned
            else if (kind == 2) { lo[a] = ri(0, dim[a] - 1); hi[a] = lo[a] + 1; }                               // one voxel
            else if (kind == 3) { const int n = ri(1, dim[a] < 12 ? dim[a] : 12); lo[a] = (rng() & 1) ? 0 : dim[a] - n; hi[a] = lo[a] + n; }   // a corner of the volume
            else if (kind == 4) { lo[a] = 0; hi[a] = dim[a]; }                                                  // the whole volume
            else { const int c = ri(0, S.nb[a] - 1) * 8 + ri(0, 1) * 8; lo[a] = c > 2 ? c - ri(1, 2) : 0; hi[a] = c + ri(1, 2) < dim[a] ? c + ri(1, 2) : dim[a]; if (hi[a] <= lo[a]) hi[a] = lo[a] + 1; }   // straddling brick faces
        }
        out[11] |= 1u << kind;
        Scene N = S;
        const int fill = ri(-2, 3);                             // carve (half of the edits), sparse, mixed, fill
        for (int z = lo[2]; z < hi[2]; z++) for (int y = lo[1]; y < hi[1]; y++) for (int x = lo[0]; x < hi[0]; x++)
            N.vox[(size_t)x + ((size_t)y + (size_t)z * N.H()) * N.W()] = fill <= 0 ? 0 : (fill == 3 || (int)(rng() % 100) < (fill == 1 ? 2 : 40)) ? (uint8_t)ri(1, 255) : 0;
        Built B0, B1;
        build(S, with_fine, B0);
        build(N, with_fine, B1);
        out[0]++;
        if (with_fine) out[10]++;
        EditSpan T[3], F[3];
        for (int a = 0; a < 3; a++) { T[a] = brick_span_t(lo[a], hi[a]); F[a] = brick_span_f(T[a], S.nb[a]); }
        bool changed = false, emptied = false, created = false;
        for (int z = 0; z < S.nb[2]; z++) for (int y = 0; y < S.nb[1]; y++) for (int x = 0; x < S.nb[0]; x++) {
            const size_t b = S.bi(x, y, z);
            if (B0.occ[b] != B1.occ[b]) {
                changed = true;
                if (B0.occ[b]) emptied = true; else created = true;
                if (!inside(T, x, y, z)) out[2]++;
            }
            if (with_fine && !inside(F, x, y, z))
                for (size_t i = 0; i < 4096; i++) if (B0.fine[b * 4096 + i] != B1.fine[b * 4096 + i]) out[1]++;
        }
        if (emptied) out[12]++;
        if (created) out[13]++;
        if (!changed) {
            for (int o = 0; o < 8; o++) if (B0.coarse[o] != B1.coarse[o]) out[6]++;
            if (B0.entry != B1.entry) out[6]++;
            continue;
        }
        out[8]++;
        if (!brick_edit_in_place(S.nb[0], S.nb[1], S.nb[2], lo, hi)) out[9]++;
        std::vector<uint8_t> in_any_q(S.nbricks(), 0);
        for (int o = 0; o < 8; o++) {
            EditSpan R[3], Q[3];
            for (int a = 0; a < 3; a++) { const int sg = ((o >> a) & 1) ? 1 : -1; R[a] = brick_span_r(T[a], S.nb[a], sg); Q[a] = brick_span_q(T[a], S.nb[a], sg); }
            for (int z = 0; z < S.nb[2]; z++) for (int y = 0; y < S.nb[1]; y++) for (int x = 0; x < S.nb[0]; x++) {
                const uint8_t a0 = B0.coarse[o][S.bi(x, y, z)], a1 = B1.coarse[o][S.bi(x, y, z)];
                if ((a0 & 0x7F) != (a1 & 0x7F) && !inside(R, x, y, z)) out[3]++;
                if ((a0 & 0x80) != (a1 & 0x80) && !inside(Q, x, y, z)) out[4]++;
                if (inside(Q, x, y, z)) in_any_q[S.bi(x, y, z)] = 1;
            }
            std::vector<uint8_t> f = B0.coarse[o];
            update_coarse(S, B1.occ, o, T, f);
            if (f != B1.coarse[o]) out[7]++;
        }
        for (size_t b = 0; b < S.nbricks(); b++) if (B0.entry[b] != B1.entry[b] && !in_any_q[b]) out[5]++;
    }
}

int brick_edit_in_place_c(int nbx, int nby, int nbz, const int lo[3], const int hi[3]) { return brick_edit_in_place(nbx, nby, nbz, lo, hi) ? 1 : 0; }

// spans[0..2] T, [3..5] F, then per octant o: [6 + 9 o ..] R_o x y z, E x y z, Q_o x y z -- each as (lo, hi)
void brick_edit_spans(int nbx, int nby, int nbz, const int lo[3], const int hi[3], int spans[78][2])
{
    const int nb[3] = {nbx, nby, nbz};
    for (int a = 0; a < 3; a++) {
        const EditSpan t = brick_span_t(lo[a], hi[a]), f = brick_span_f(t, nb[a]);
        spans[a][0] = t.lo; spans[a][1] = t.hi; spans[3 + a][0] = f.lo; spans[3 + a][1] = f.hi;
        for (int o = 0; o < 8; o++) {
            const int sg = ((o >> a) & 1) ? 1 : -1;
            const EditSpan r = brick_span_r(t, nb[a], sg), e = brick_span_e(t, nb[a]), q = brick_span_q(t, nb[a], sg);
            spans[6 + 9 * o + a][0] = r.lo; spans[6 + 9 * o + a][1] = r.hi;
            spans[6 + 9 * o + 3 + a][0] = e.lo; spans[6 + 9 * o + 3 + a][1] = e.hi;
            spans[6 + 9 * o + 6 + a][0] = q.lo; spans[6 + 9 * o + 6 + a][1] = q.hi;
        }
    }
}

}
