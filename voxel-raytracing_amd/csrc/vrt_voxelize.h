// vrt_voxelize.h -- which voxels a triangle mesh covers (vrt_scene_voxelize).  Plain integer arithmetic, no floating point
// anywhere: coverage is a function of integers, so the device (vrt_voxelize.hip), the host (vrt_api_edit.hip) and the tests
// (tests/native/voxelize_host.cpp, held against Python integers) agree bit for bit by construction.
//
// UNITS.  Positions are in SIXTEENTHS of a voxel (VRT_VOXELIZE_UNIT).  Voxel (x, y, z) is the closed cube [16x, 16x+16]^3, its
// centre c = (16x+8, 16y+8, 16z+8), its half-side h = 8 (VRT_VOXELIZE_HALF).
//
// INPUT.  vertices int32[nv][3], triangles uint32[nt][3] (indices), nt in 1..2^20, nv in 1..2^24, every coordinate in
// -65536..131072 (-4096..8192 voxels).  A candidate voxel always lies inside the volume (0..4095), so its centre is in 8..65528.
//
// WHAT FITS WHERE (e_i = v_(i+1) - v_i, n = e0 x e1):
//   |v - c| per component <= max(131072 - 8, 65536 + 65528) = 131064 < 2^18
//   |e| per component     <= 196608 < 2^18
//   |n| per component     <= 2 * 196608^2 < 2^37
//   |n . (v - c)|         <= 3 * 2^37 * 2^18 < 2^57;   h (|nx| + |ny| + |nz|) < 2^42
//   the nine edge axes k = e_i x unit axis have two components of e: |k . (v - c)| <= 2 * 2^18 * 2^18 = 2^37, r = h |k|_1 < 2^22
//   the top-left rule's E = dy (cz - az) - dz (cy - ay): < 2^37
//   the crossing count: A = |nx| < 2^37, 16 A < 2^41, T = -(B + A (16 x0 + 8 - v0x)) with |T| < 2^57 (it is an n . (c - v0))
// Everything fits int64_t; nothing needs 128 bits.
//
// SURFACE (conservative).  Voxel and triangle meet iff none of the 13 axes separates them, closed comparisons:
//   the three box axes        min_i (v_i - c)_a <= h and max_i (v_i - c)_a >= -h
//   the triangle's normal     |n . (v0 - c)| <= h (|nx| + |ny| + |nz|)
//   the nine k = e_i x axis   the interval of k . (v_j - c), j = 0..2, meets [-r, r], r = h (|kx| + |ky| + |kz|)
// A degenerate triangle (a segment, a point) comes out right under the same rules: its zero normal passes trivially.  Of the 13
// axes, the y and z box axes and the three e_i x X depend on (y, z) only: vox_row_meets.  The other eight: vox_lane_meets.
//
// SOLID (centre parity along +x).  A triangle with nx == 0 flips nothing.  Otherwise, s = sign(nx), it flips the voxel of centre c
// iff (a) c lies in its yz-projection under a top-left rule -- for each edge a -> b, dy = s (by - ay), dz = s (bz - az),
// E = dy (cz - az) - dz (cy - ay): E > 0 passes, E == 0 passes iff dz > 0 or (dz == 0 and dy < 0) -- and (b) s (n . (c - v0)) < 0,
// strictly.  A voxel is inside iff an odd number of triangles flip it.  s nx > 0, so along a row (b) holds for a PREFIX of the
// voxels: vox_cross_count says how long it is, by one division and a correction checked against the exact comparison.
// Triangles outside the bounds count: one whose crossing lies beyond the high x end of a row flips the whole row.  Therefore a
// solid voxelized in parts (any split of the bounds) gives the same voxels as in one piece.
//
// MASKS, over the clipped bounds [clo, clo + csize), x fastest, 64-bit words, row (by, bz) -> by + bz * csize[1]:
//   coverage  vox_cover_words(csize[0]) words per row, bit bx & 63 of word bx >> 6
//   toggle    vox_toggle_words(csize[0]) words per row, bits 0..csize[0]: bit k set = an odd number of triangles flip the voxels
//             bx < k of the row (bit csize[0]: the whole row).  inside(bx) = the XOR of the bits above bx (vox_scan_word).
//
// WORK.  The host cuts every triangle's clipped box into items (triangle, first row, rows) of at most `item_rows` rows of at most
// 8 words (VRT_VOXELIZE_ITEM_ROWS unless lowered), so no wave's work grows with a triangle; SOLID has its own items over the
// columns of the yz-box.  Candidates: over the triangles, the voxels of their clipped boxes (SURFACE) plus the columns of their
// clipped yz-boxes (SOLID); above VRT_VOXELIZE_MAX_CANDIDATES, or VRT_VOXELIZE_MAX_ITEMS items, the call is refused
// (VRT_ERR_UNSUPPORTED) and changes nothing.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define VRT_VOX_HD __host__ __device__ inline
#define VRT_VOX_UNROLL _Pragma("unroll")     // the loops over three: a triangle in registers, not in private memory
#else
#define VRT_VOX_HD inline
#define VRT_VOX_UNROLL
#endif

#define VRT_VOXELIZE_UNIT 16
#define VRT_VOXELIZE_HALF 8
#define VRT_VOXELIZE_COORD_MIN (-65536)
#define VRT_VOXELIZE_COORD_MAX 131072
#define VRT_VOXELIZE_MAX_TRIANGLES (1u << 20)
#define VRT_VOXELIZE_MAX_VERTICES (1u << 24)
#define VRT_VOXELIZE_MAX_SIDE 512u
#define VRT_VOXELIZE_MAX_SIZE (1u << 30)
// (include/vrt.h has the same values for the C-ABI; vrt_api_edit.hip asserts that they agree)
#define VRT_VOXELIZE_FILL_SURFACE 1u
#define VRT_VOXELIZE_FILL_SOLID 2u
#define VRT_VOXELIZE_MAX_CANDIDATES (1ull << 31)   // the most candidate voxels (and columns) one call may test
#define VRT_VOXELIZE_MAX_ITEMS (1u << 24)             // the most work items of one call (beyond: refused, as above)
#define VRT_VOXELIZE_ITEM_ROWS 64u                 // rows (SURFACE) or groups of 64 columns (SOLID) of one work item

namespace vrt {

struct VoxTri {
    int32_t v[3][3];     // the vertices
    int32_t e[3][3];     // e[i] = v[(i + 1) % 3] - v[i]
    int64_t n[3];        // e[0] x e[1]
    int64_t nr;          // h (|nx| + |ny| + |nz|)
};

// one work item: rows [first, first + count) of the triangle's clipped yz-box (row = (y - y0) + (z - z0) * ny)
struct VoxItem { uint32_t tri, first, count; };

VRT_VOX_HD int64_t vox_abs(int64_t v) { return v < 0 ? -v : v; }
VRT_VOX_HD int32_t vox_floor_div16(int32_t v) { return v >= 0 ? v / 16 : -((15 - v) / 16); }
VRT_VOX_HD int32_t vox_centre(int32_t voxel) { return VRT_VOXELIZE_UNIT * voxel + VRT_VOXELIZE_HALF; }
VRT_VOX_HD bool vox_coord_ok(int32_t v) { return v >= VRT_VOXELIZE_COORD_MIN && v <= VRT_VOXELIZE_COORD_MAX; }

// the voxels whose closed cube meets [m, M] on one axis: *lo .. *hi, both inclusive
VRT_VOX_HD void vox_axis_span(int32_t m, int32_t M, int32_t* lo, int32_t* hi)
{
    *lo = vox_floor_div16(m + 15) - 1;     // ceil(m / 16) - 1
    *hi = vox_floor_div16(M);
}

VRT_VOX_HD bool vox_job_ok(int32_t mode, uint32_t id, uint32_t match, uint32_t fill, const uint32_t size[3])
{
    if (fill == 0u || (fill & ~(VRT_VOXELIZE_FILL_SURFACE | VRT_VOXELIZE_FILL_SOLID)) != 0u) return false;
    VRT_VOX_UNROLL
    for (int a = 0; a < 3; a++)
        if (size[a] < 1u || size[a] > VRT_VOXELIZE_MAX_SIZE) return false;
    if (mode == 0) return true;                                 // VRT_BRUSH_MODE_SET .. REPLACE, as brush_mode_ok
    if (mode == 1 || mode == 2) return id != 0u;
    if (mode == 3) return id != match;
    return false;
}

VRT_VOX_HD bool vox_sides_ok(const uint32_t csize[3])
{
    return csize[0] <= VRT_VOXELIZE_MAX_SIDE && csize[1] <= VRT_VOXELIZE_MAX_SIDE && csize[2] <= VRT_VOXELIZE_MAX_SIDE;
}

VRT_VOX_HD uint32_t vox_cover_words(uint32_t size_x) { return (size_x + 63u) / 64u; }
VRT_VOX_HD uint32_t vox_toggle_words(uint32_t size_x) { return size_x / 64u + 1u; }
VRT_VOX_HD size_t vox_row_index(uint32_t by, uint32_t bz, const uint32_t csize[3]) { return (size_t)by + (size_t)bz * (size_t)csize[1]; }

VRT_VOX_HD void vox_tri_setup(const int32_t* a, const int32_t* b, const int32_t* c, VoxTri& T)
{
    VRT_VOX_UNROLL
    for (int k = 0; k < 3; k++) {
        T.v[0][k] = a[k]; T.v[1][k] = b[k]; T.v[2][k] = c[k];
        T.e[0][k] = b[k] - a[k]; T.e[1][k] = c[k] - b[k]; T.e[2][k] = a[k] - c[k];
    }
    T.n[0] = (int64_t)T.e[0][1] * T.e[1][2] - (int64_t)T.e[0][2] * T.e[1][1];
    T.n[1] = (int64_t)T.e[0][2] * T.e[1][0] - (int64_t)T.e[0][0] * T.e[1][2];
    T.n[2] = (int64_t)T.e[0][0] * T.e[1][1] - (int64_t)T.e[0][1] * T.e[1][0];
    T.nr = VRT_VOXELIZE_HALF * (vox_abs(T.n[0]) + vox_abs(T.n[1]) + vox_abs(T.n[2]));
}

// The triangle's box of voxels cut to the clipped bounds: lo .. hi inclusive.  false: it meets no voxel of the bounds.
// solid: the box of the columns a crossing can flip instead -- the yz-box, every x of the bounds; false also when nx == 0 or
// the triangle lies wholly at or below the first centre of the rows (it can flip no voxel of them).
VRT_VOX_HD bool vox_tri_box(const VoxTri& T, bool solid, const int32_t clo[3], const uint32_t csize[3], int32_t lo[3], int32_t hi[3])
{
    VRT_VOX_UNROLL
    for (int a = 0; a < 3; a++) {
        int32_t m = T.v[0][a], M = T.v[0][a];
        VRT_VOX_UNROLL
        for (int i = 1; i < 3; i++) { m = T.v[i][a] < m ? T.v[i][a] : m; M = T.v[i][a] > M ? T.v[i][a] : M; }
        const int32_t blo = clo[a], bhi = clo[a] + (int32_t)csize[a] - 1;
        if (solid && a == 0) {
            if (T.n[0] == 0 || M <= vox_centre(blo)) return false;
            lo[a] = blo; hi[a] = bhi;
            continue;
        }
        vox_axis_span(m, M, &lo[a], &hi[a]);                     // (solid: a centre inside [m, M] is a voxel of this span, so the same box serves)
        lo[a] = lo[a] < blo ? blo : lo[a];
        hi[a] = hi[a] > bhi ? bhi : hi[a];
        if (hi[a] < lo[a]) return false;
    }
    return true;
}

// the interval [min p, max p] meets [-r, r]
VRT_VOX_HD bool vox_axis_meets(int64_t p0, int64_t p1, int64_t p2, int64_t r)
{
    const int64_t mn = p0 < p1 ? (p0 < p2 ? p0 : p2) : (p1 < p2 ? p1 : p2), mx = p0 > p1 ? (p0 > p2 ? p0 : p2) : (p1 > p2 ? p1 : p2);
    return mn <= r && mx >= -r;
}

// SURFACE, the five axes that depend on (y, z) only: the y and z box axes and e_i x X = (0, e_z, -e_y)
VRT_VOX_HD bool vox_row_meets(const VoxTri& T, int32_t cy, int32_t cz)
{
    if (!vox_axis_meets(T.v[0][1] - cy, T.v[1][1] - cy, T.v[2][1] - cy, VRT_VOXELIZE_HALF)) return false;
    if (!vox_axis_meets(T.v[0][2] - cz, T.v[1][2] - cz, T.v[2][2] - cz, VRT_VOXELIZE_HALF)) return false;
    VRT_VOX_UNROLL
    for (int i = 0; i < 3; i++) {
        const int64_t ky = T.e[i][2], kz = -(int64_t)T.e[i][1];
        const int64_t p0 = ky * (T.v[0][1] - cy) + kz * (T.v[0][2] - cz), p1 = ky * (T.v[1][1] - cy) + kz * (T.v[1][2] - cz),
                      p2 = ky * (T.v[2][1] - cy) + kz * (T.v[2][2] - cz);
        if (!vox_axis_meets(p0, p1, p2, VRT_VOXELIZE_HALF * (vox_abs(ky) + vox_abs(kz)))) return false;
    }
    return true;
}

// SURFACE, the other eight: the x box axis, the normal, e_i x Y = (-e_z, 0, e_x) and e_i x Z = (e_y, -e_x, 0)
VRT_VOX_HD bool vox_lane_meets(const VoxTri& T, int32_t cx, int32_t cy, int32_t cz)
{
    if (!vox_axis_meets(T.v[0][0] - cx, T.v[1][0] - cx, T.v[2][0] - cx, VRT_VOXELIZE_HALF)) return false;
    const int64_t d[3][3] = {{T.v[0][0] - cx, T.v[0][1] - cy, T.v[0][2] - cz}, {T.v[1][0] - cx, T.v[1][1] - cy, T.v[1][2] - cz},
                             {T.v[2][0] - cx, T.v[2][1] - cy, T.v[2][2] - cz}};
    if (vox_abs(T.n[0] * d[0][0] + T.n[1] * d[0][1] + T.n[2] * d[0][2]) > T.nr) return false;
    VRT_VOX_UNROLL
    for (int i = 0; i < 3; i++) {
        const int64_t ex = T.e[i][0], ey = T.e[i][1], ez = T.e[i][2];
        if (!vox_axis_meets(-ez * d[0][0] + ex * d[0][2], -ez * d[1][0] + ex * d[1][2], -ez * d[2][0] + ex * d[2][2],
                            VRT_VOXELIZE_HALF * (vox_abs(ez) + vox_abs(ex)))) return false;
        if (!vox_axis_meets(ey * d[0][0] - ex * d[0][1], ey * d[1][0] - ex * d[1][1], ey * d[2][0] - ex * d[2][1],
                            VRT_VOXELIZE_HALF * (vox_abs(ey) + vox_abs(ex)))) return false;
    }
    return true;
}

VRT_VOX_HD bool vox_meets(const VoxTri& T, int32_t x, int32_t y, int32_t z)
{
    return vox_row_meets(T, vox_centre(y), vox_centre(z)) && vox_lane_meets(T, vox_centre(x), vox_centre(y), vox_centre(z));
}

// SOLID.  sign(nx)
VRT_VOX_HD int vox_cross_sign(const VoxTri& T) { return T.n[0] > 0 ? 1 : (T.n[0] < 0 ? -1 : 0); }

// rule (a): the centre's column lies in the yz-projection, top-left rule; s != 0
VRT_VOX_HD bool vox_column_inside(const VoxTri& T, int s, int32_t cy, int32_t cz)
{
    VRT_VOX_UNROLL
    for (int i = 0; i < 3; i++) {
        const int64_t dy = (int64_t)s * T.e[i][1], dz = (int64_t)s * T.e[i][2];
        const int64_t E = dy * (cz - T.v[i][2]) - dz * (cy - T.v[i][1]);
        if (E < 0) return false;
        if (E == 0 && !(dz > 0 || (dz == 0 && dy < 0))) return false;
    }
    return true;
}

// rule (b)'s left side: s (n . (c - v0))
VRT_VOX_HD int64_t vox_plane(const VoxTri& T, int s, int32_t cx, int32_t cy, int32_t cz)
{
    return (int64_t)s * (T.n[0] * (cx - T.v[0][0]) + T.n[1] * (cy - T.v[0][1]) + T.n[2] * (cz - T.v[0][2]));
}

VRT_VOX_HD bool vox_flips(const VoxTri& T, int32_t x, int32_t y, int32_t z)
{
    const int s = vox_cross_sign(T);
    if (s == 0) return false;
    return vox_column_inside(T, s, vox_centre(y), vox_centre(z)) && vox_plane(T, s, vox_centre(x), vox_centre(y), vox_centre(z)) < 0;
}

// how many of the voxels x0 .. x0 + size_x - 1 of the row (cy, cz) satisfy (b): they are the first `count` of them; s != 0
VRT_VOX_HD uint32_t vox_cross_count(const VoxTri& T, int s, int32_t x0, uint32_t size_x, int32_t cy, int32_t cz)
{
    const int64_t A16 = 16 * (int64_t)s * T.n[0];                 // > 0: what one voxel along x adds to the plane's value
    const int64_t t = -vox_plane(T, s, vox_centre(x0), cy, cz);  // voxel i satisfies (b) iff A16 * i < t
    int64_t k = t > 0 ? t / A16 : 0;
    if (k > (int64_t)size_x) k = (int64_t)size_x;
    if (k < (int64_t)size_x && A16 * k < t) k++;                 // the quotient was rounded down: at most one more
    if (k > 0 && !(A16 * (k - 1) < t)) k--;                      // (never taken; the exact comparison decides)
    return (uint32_t)k;
}

// One word of a row's scan, from the highest word down.  t: the toggle word; *carry: the XOR of every bit above this word (in: of
// the words above, out: this word included).  Returns inside() for the word's 64 voxels, before masking to the row's length.
VRT_VOX_HD uint64_t vox_scan_word(uint64_t t, uint64_t* carry)
{
    uint64_t sfx = t;                                            // bit i: the XOR of bits i..63
    sfx ^= sfx >> 1; sfx ^= sfx >> 2; sfx ^= sfx >> 4; sfx ^= sfx >> 8; sfx ^= sfx >> 16; sfx ^= sfx >> 32;
    const uint64_t inside = (sfx >> 1) ^ (*carry ? ~0ull : 0ull);
    *carry ^= sfx & 1ull;
    return inside;
}

// the bits of coverage word w that are voxels of a row of size_x
VRT_VOX_HD uint64_t vox_word_valid(uint32_t w, uint32_t size_x)
{
    const uint32_t left = size_x - w * 64u;
    return left >= 64u ? ~0ull : ((1ull << left) - 1ull);
}

} // namespace vrt
