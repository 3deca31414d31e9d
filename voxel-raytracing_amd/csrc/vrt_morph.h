// vrt_morph.h -- binary morphology of a scene's occupancy (vrt_scene_morph): which voxels growing, shrinking, opening, closing
// or hollowing the solid adds and removes, and how the device finds them.  Plain integer arithmetic, compiled for the device
// (vrt_morph.hip), the host (vrt_api_edit.hip) and the tests (tests/native/morph_host.cpp, morph_fuzz.cpp, held against two
// definitions in Python integers, tests/morph_reference.py).
//
// DEFINITION.  S is the set of solid cells (id != 0) of the INFINITE grid: inside the volume what the scene holds, outside the
// volume every cell empty -- or, with VRT_MORPH_FLAG_BORDER_SOLID, every cell solid.  The distance between two cells is L1 under
// VRT_MORPH_CONN_FACES = 6 and L-infinity under VRT_MORPH_CONN_CORNERS = 26; the radius r is in 1..VRT_MORPH_MAX_RADIUS = 8.
//     dil_r(X) = { v : some x in X with dist(v, x) <= r }
//     ero_r(X) = { v : every u with dist(v, u) <= r is in X }  =  complement of dil_r(complement of X)
// Both equal r applications of the UNIT STEP of that connectivity (dil_1, ero_1): the ball of radius r of either distance is the
// r-fold Minkowski sum of its unit ball (tests/test_morph_cpu.py proves it on the reference for every r the API takes at its
// edges).  The RESULT SET R:
//     VRT_MORPH_OP_DILATE   dil_r(S)
//     VRT_MORPH_OP_ERODE    ero_r(S)
//     VRT_MORPH_OP_OPEN     dil_r(ero_r(S))        (R is a subset of S: removes specks)
//     VRT_MORPH_OP_CLOSE    ero_r(dil_r(S))        (S is a subset of R: closes pinholes)
//     VRT_MORPH_OP_HOLLOW   S \ ero_r(S)           (a shell of thickness r)
// R is a function of the whole grid; it is WRITTEN only inside the BOUNDS [lo, lo + size) (lo may be negative, every size in
// 1..2^30), cut to the volume with brush_clip; a clipped side above VRT_MORPH_MAX_SIDE = 512 is refused.  Of the clipped bounds
//     an empty voxel in R becomes `id`;  a solid voxel not in R becomes 0;  every other voxel keeps its id        (morph_value)
// -- morphology never recolours.  DILATE and CLOSE need id >= 1; ERODE, OPEN and HOLLOW cannot add a voxel and ignore the id.
//
// THE HALO.  Cells of the volume outside the bounds are read as they are.  A cell of R depends on S within distance
// h = morph_halo: r for the one-phase operations (DILATE, ERODE, HOLLOW), 2r for OPEN and CLOSE.  So one operation done in parts
// over the same old scene agrees with the whole (parts applied in place one after another do not: a later part reads what an
// earlier one wrote).
//
// LAYOUT.  The DOMAIN is the clipped bounds grown by h on every side, beyond the volume where that leads: low corner
// mlo[a] = clo[a] - h, sides msize[a] = csize[a] + 2h <= 544 (morph_domain).  A MASK over the domain holds one bit per cell, in
// rows along x of 32-bit ROW WORDS (one LDS bank wide: consecutive lanes on consecutive words never conflict): the cell at offset
// (mx, my, mz) from mlo is bit mx & 31 of word
//     (mx >> 5) + nw * (my + msize[1] * mz),     nw = ceil(msize[0] / 32) <= 17                       (morph_word_index)
// Bits of a row's last word beyond msize[0] hold nothing that is ever read as a cell.  Two masks of 544^3 bits are 2 x 20.9 MB.
//   1. the MASK PASS writes S over the domain into mask A: a lane per cell, the wave's ballot is two row words.
//   2. a PHASE is dil_r or ero_r of one mask into the other: DILATE [dil], ERODE and HOLLOW [ero], OPEN [ero, dil], CLOSE
//      [dil, ero] (morph_phase_erodes); the result is mask B after one phase, mask A after two.  Erosion is the same dilation run
//      on the complement: the words are complemented as they are loaded and as they are stored.
//   3. the extent and compose kernels read the cell's bit and the voxel: in R iff the bit (HOLLOW: solid and not the bit).
//
// ONE PHASE, TILED.  A workgroup takes a TILE of VRT_MORPH_TILE_WORDS = 2 row words x 16 x 16 rows of the domain and loads its
// EXTENDED block: one more word on either side in x (32 cells >= r) and r more rows on either side in y and z, E = 16 + 2r <= 32
// rows per axis, word (xw, ey, ez) at xw + 4 * (ey + E * ez) (morph_ext_index); what lies outside the domain is loaded as 0.  It
// then runs the r unit steps in place of r launches (morph_ext_step; two buffers taken in turn):
//     6:   row | row << 1 | row >> 1 (with the carry bits of the neighbour words) | the rows at y - 1, y + 1, z - 1, z + 1
//     26:  u = the OR of the nine rows (y - 1..y + 1) x (z - 1..z + 1);  u | u << 1 | u >> 1 (with the carries)
// EXACTNESS.  After k unit steps the value of a cell is a function of the initial values within distance k of it, and of nothing
// else (induction over k: one step reads distance 1).  A cell of the tile lies at least r rows from the block's faces in y and z
// and at least 32 >= r cells from them in x, so its ball of radius r is inside the block: after r steps it holds dil_r exactly,
// whatever was assumed beyond the block.  Step k (1-based) therefore computes only the rows k .. E - 1 - k of y and z, which is
// what step k + 1 reads.  The same argument across phases: R at a cell of the clipped bounds reads the first phase's mask within
// r of it, which reads S within r of that -- all inside the domain, where the mask pass wrote S of the infinite grid.  Cells of
// the first phase's mask nearer than r to the domain's faces are not exact, and are at distance > r from every cell of the bounds.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define VRT_MORPH_HD __host__ __device__ inline
#else
#define VRT_MORPH_HD inline
#endif

// (include/vrt.h has the same values for the C-ABI; vrt_api_edit.hip asserts that they agree)
#define VRT_MORPH_OP_DILATE 0
#define VRT_MORPH_OP_ERODE 1
#define VRT_MORPH_OP_OPEN 2
#define VRT_MORPH_OP_CLOSE 3
#define VRT_MORPH_OP_HOLLOW 4
#define VRT_MORPH_CONN_FACES 6
#define VRT_MORPH_CONN_CORNERS 26
#define VRT_MORPH_FLAG_BORDER_SOLID 1u
#define VRT_MORPH_FLAG_MEASURE 2u

#define VRT_MORPH_MAX_RADIUS 8
#define VRT_MORPH_MAX_SIDE 512u           // voxels, of the clipped bounds
#define VRT_MORPH_MAX_SIZE (1u << 30)     // of the bounds as given
#define VRT_MORPH_TILE_WORDS 2u           // row words of a tile
#define VRT_MORPH_TILE_ROWS 16u           // rows of a tile along y and along z
#define VRT_MORPH_EXT_WORDS 4u            // row words of an extended block
#define VRT_MORPH_EXT_MAX 4096u           // words of the largest extended block: 4 * 32 * 32

namespace vrt {

VRT_MORPH_HD bool morph_adds(int32_t op) { return op == VRT_MORPH_OP_DILATE || op == VRT_MORPH_OP_CLOSE; }

VRT_MORPH_HD bool morph_args_ok(int32_t op, int32_t connectivity, int32_t radius, uint32_t flags, uint32_t id, const uint32_t size[3])
{
    if (op < VRT_MORPH_OP_DILATE || op > VRT_MORPH_OP_HOLLOW) return false;
    if (connectivity != VRT_MORPH_CONN_FACES && connectivity != VRT_MORPH_CONN_CORNERS) return false;
    if (radius < 1 || radius > VRT_MORPH_MAX_RADIUS) return false;
    if (flags & ~(VRT_MORPH_FLAG_BORDER_SOLID | VRT_MORPH_FLAG_MEASURE)) return false;
    if (morph_adds(op) && (id < 1u || id > 255u)) return false;
    for (int a = 0; a < 3; a++)
        if (size[a] < 1u || size[a] > VRT_MORPH_MAX_SIZE) return false;
    return true;
}

VRT_MORPH_HD bool morph_sides_ok(const uint32_t csize[3])
{
    return csize[0] <= VRT_MORPH_MAX_SIDE && csize[1] <= VRT_MORPH_MAX_SIDE && csize[2] <= VRT_MORPH_MAX_SIDE;
}

VRT_MORPH_HD uint32_t morph_phases(int32_t op) { return (op == VRT_MORPH_OP_OPEN || op == VRT_MORPH_OP_CLOSE) ? 2u : 1u; }
VRT_MORPH_HD uint32_t morph_halo(int32_t op, int32_t radius) { return morph_phases(op) * (uint32_t)radius; }
// is phase p (0 or 1) of the operation an erosion?
VRT_MORPH_HD bool morph_phase_erodes(int32_t op, uint32_t p)
{
    if (op == VRT_MORPH_OP_OPEN) return p == 0u;
    if (op == VRT_MORPH_OP_CLOSE) return p == 1u;
    return op != VRT_MORPH_OP_DILATE;
}

// the domain of the masks: the clipped bounds grown by the halo
VRT_MORPH_HD void morph_domain(const int32_t clo[3], const uint32_t csize[3], uint32_t halo, int32_t mlo[3], uint32_t msize[3])
{
    for (int a = 0; a < 3; a++) { mlo[a] = clo[a] - (int32_t)halo; msize[a] = csize[a] + 2u * halo; }
}

VRT_MORPH_HD uint32_t morph_row_words(uint32_t msize_x) { return (msize_x + 31u) / 32u; }
VRT_MORPH_HD size_t morph_mask_words(const uint32_t msize[3]) { return (size_t)morph_row_words(msize[0]) * (size_t)msize[1] * (size_t)msize[2]; }
VRT_MORPH_HD size_t morph_word_index(uint32_t wx, uint32_t my, uint32_t mz, const uint32_t msize[3])
{
    return (size_t)wx + (size_t)morph_row_words(msize[0]) * ((size_t)my + (size_t)msize[1] * (size_t)mz);
}
// the bit of the cell at offset (mx, my, mz) from the domain's low corner
VRT_MORPH_HD bool morph_mask_bit(const uint32_t* mask, uint32_t mx, uint32_t my, uint32_t mz, const uint32_t msize[3])
{
    return ((mask[morph_word_index(mx >> 5, my, mz, msize)] >> (mx & 31u)) & 1u) != 0u;
}

// tiles of the domain per axis
VRT_MORPH_HD void morph_tiles(const uint32_t msize[3], uint32_t nt[3])
{
    nt[0] = (morph_row_words(msize[0]) + VRT_MORPH_TILE_WORDS - 1u) / VRT_MORPH_TILE_WORDS;
    nt[1] = (msize[1] + VRT_MORPH_TILE_ROWS - 1u) / VRT_MORPH_TILE_ROWS;
    nt[2] = (msize[2] + VRT_MORPH_TILE_ROWS - 1u) / VRT_MORPH_TILE_ROWS;
}

VRT_MORPH_HD uint32_t morph_ext_rows(uint32_t r) { return VRT_MORPH_TILE_ROWS + 2u * r; }
VRT_MORPH_HD uint32_t morph_ext_count(uint32_t r) { return VRT_MORPH_EXT_WORDS * morph_ext_rows(r) * morph_ext_rows(r); }
VRT_MORPH_HD uint32_t morph_ext_index(uint32_t xw, uint32_t ey, uint32_t ez, uint32_t E) { return xw + VRT_MORPH_EXT_WORDS * (ey + E * ez); }

// word i of tile (tx, ty, tz)'s extended block, from the mask src: 0 outside the domain, complemented for an erosion
VRT_MORPH_HD uint32_t morph_ext_load(const uint32_t* src, const uint32_t msize[3], bool erode, uint32_t tx, uint32_t ty, uint32_t tz, uint32_t r, uint32_t i)
{
    const uint32_t E = morph_ext_rows(r), xw = i % VRT_MORPH_EXT_WORDS, row = i / VRT_MORPH_EXT_WORDS, ey = row % E, ez = row / E;
    const int64_t gw = (int64_t)tx * VRT_MORPH_TILE_WORDS + xw - 1, gy = (int64_t)ty * VRT_MORPH_TILE_ROWS + ey - r, gz = (int64_t)tz * VRT_MORPH_TILE_ROWS + ez - r;
    uint32_t v = 0u;
    if (gw >= 0 && gw < (int64_t)morph_row_words(msize[0]) && gy >= 0 && gy < (int64_t)msize[1] && gz >= 0 && gz < (int64_t)msize[2])
        v = src[morph_word_index((uint32_t)gw, (uint32_t)gy, (uint32_t)gz, msize)];
    return erode ? ~v : v;
}

// does step k (1..r) compute row (ey, ez) of the extended block?  The rows that step k + 1 reads, and the tile's at k = r.
VRT_MORPH_HD bool morph_ext_live(uint32_t E, uint32_t k, uint32_t ey, uint32_t ez) { return ey >= k && ey + k < E && ez >= k && ez + k < E; }

// what word (xw, ey, ez), a live row of step k >= 1 (so the rows beside it exist), becomes under one unit dilation of ext
VRT_MORPH_HD uint32_t morph_ext_step(int connectivity, const uint32_t* ext, uint32_t E, uint32_t xw, uint32_t ey, uint32_t ez)
{
    const uint32_t sy = VRT_MORPH_EXT_WORDS, sz = VRT_MORPH_EXT_WORDS * E;
    const uint32_t* c = ext + morph_ext_index(xw, ey, ez, E);
    const bool left = xw > 0u, right = xw + 1u < VRT_MORPH_EXT_WORDS;
    if (connectivity == VRT_MORPH_CONN_FACES) {
        const uint32_t w = c[0];
        return w | (w << 1) | (w >> 1) | (left ? c[-1] >> 31 : 0u) | (right ? c[1] << 31 : 0u) | c[-(int)sy] | c[sy] | c[-(int)sz] | c[sz];
    }
    uint32_t u = 0u, ul = 0u, ur = 0u;
    for (int dz = -1; dz <= 1; dz++) for (int dy = -1; dy <= 1; dy++) {
        const uint32_t* p = c + dy * (int)sy + dz * (int)sz;
        u |= p[0];
        if (left) ul |= p[-1];
        if (right) ur |= p[1];
    }
    return u | (u << 1) | (u >> 1) | (ul >> 31) | (ur << 31);
}

// the r unit steps of one tile on the host: a holds the extended block, b is room for another; -> the buffer that holds the result
VRT_MORPH_HD uint32_t* morph_tile_run(int connectivity, uint32_t r, uint32_t* a, uint32_t* b)
{
    const uint32_t E = morph_ext_rows(r), n = morph_ext_count(r);
    for (uint32_t k = 1; k <= r; k++) {
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t xw = i % VRT_MORPH_EXT_WORDS, row = i / VRT_MORPH_EXT_WORDS, ey = row % E, ez = row / E;
            if (morph_ext_live(E, k, ey, ez)) b[i] = morph_ext_step(connectivity, a, E, xw, ey, ez);
        }
        uint32_t* t = a; a = b; b = t;
    }
    return a;
}

// is the voxel in R?  bit: its bit of the result mask; solid: its id != 0
VRT_MORPH_HD bool morph_in_result(int32_t op, bool bit, bool solid) { return op == VRT_MORPH_OP_HOLLOW ? (solid && !bit) : bit; }

// what a voxel of the clipped bounds becomes
VRT_MORPH_HD uint32_t morph_value(int32_t op, bool bit, uint32_t old, uint32_t id)
{
    const bool in = morph_in_result(op, bit, old != 0u);
    return (in && old == 0u) ? id : (!in && old != 0u) ? 0u : old;
}

} // namespace vrt
