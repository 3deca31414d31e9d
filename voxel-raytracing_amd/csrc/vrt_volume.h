// vrt_volume.h -- what a march reads and what it returns, host + device: the traversal constants, VolumeView (a scene's voxel
// data: ids, occupancy pyramid, clearance fields, bricks), RayInt, the statistics hooks, the bit casts, the occupancy look-ups
// and the layout of the clearance fields (df_index and the conditions of 32-bit indexing).  No march and no assembly: this is
// the header for code that builds or hands over a VolumeView without tracing through it (vrt_internal.h, the scene build,
// the C-ABI objects).  The marches: vrt_march_*.h, behind vrt_traverse.h.
#pragma once

#include "vrt_spec.h"

#ifndef VRT_TRAVERSAL_DENSE
#define VRT_TRAVERSAL_DENSE 1
#define VRT_TRAVERSAL_BITMASK 2
#define VRT_TRAVERSAL_JUMP 3
#define VRT_TRAVERSAL_DF 4
#define VRT_TRAVERSAL_DFJ 5
#endif
#define VRT_TRAVERSAL_BRICK 6     // brick scenes (vrt_scene_from_bricks): DF over a two-level clearance; chosen by AUTO
#define VRT_TRAVERSAL_DF_FAST 7   // internal: DF through the hand-written look-up loop (trace_df_fast); chosen by the host
#define VRT_TRAVERSAL_DF_FAST_CNT 8   // internal: the same through the loops' counting twins (VRT_FLAG_MARCHED_COUNTS / VRT_FLAG_LOOKUP_COUNTS)
#define VRT_TRAVERSAL_BRICK_CNT 9     // internal: the brick march with its counters (the same flags, and every launch that fills iteration-count planes)

namespace vrt {

// Read-only view of a scene's voxel data (device pointers on the device, host pointers in the tests).
struct VolumeView {
    const uint8_t*  vox;     // W*H*D, x + y*W + z*W*H
    const uint64_t* occ1;    // per 4^3 voxels, bit (x&3)|(y&3)<<2|(z&3)<<4
    const uint64_t* occ2;    // per 16^3
    const uint64_t* occ3;    // per 64^3
    const uint8_t*  df;      // 8 octant clearance fields, each x-fastest with a one-voxel border of zeros (df_index): field o
                             // (bit0: +x, bit1: +y, bit2: +z) holds per voxel 0 = solid, else min(63, side of the largest
                             // empty cube that has this voxel as its corner and extends towards the octant's signs;
                             // outside the volume counts as solid)
    uint64_t        df_stride;  // bytes between octant fields
    uint32_t        df_fast;    // 1: the allocation continues with a ninth field, the voxel ids in the same zero-bordered layout
                                // (field 8), and one byte 0xFF at offset 9 * df_stride, and all of it is addressable with
                                // 32-bit offsets (trace_df_fast)
    uint32_t        count_lookups; // 1 (VRT_FLAG_LOOKUP_COUNTS): r.fetches holds the bytes a ray's march asked for instead of its iterations
    uint32_t        count_marched; // 1 (VRT_FLAG_MARCHED_COUNTS): an any-hit ray that is decided a miss without stepping (its clearance covers
                                // what is left of its budget) reports the iterations it TOOK, not the budget the reference's loop would
                                // have spent -- the count planes then hold the product march's own work
    // brick scenes (vrt_scene_from_bricks; vox / occ* / df are null): the volume in 8^3 bricks.  All grids are padded by one
    // brick on every side (index (bx+1) + ((by+1) + (bz+1) * pby) * pbx), the border counting as outside the volume.
    const uint32_t* bgrid;      // 0 = empty brick, 0xFFFFFFFF = border (outside the volume), else 1 + index into bpool / bfine
    const uint8_t*  bcoarse;    // 8 octant fields over the padded grid: 0 = occupied brick or border, else min(16, side in BRICKS of
                                // the largest cube of empty bricks cornered here and extending towards the octant's signs)
    uint64_t        bcoarse_stride;
    const uint8_t*  bpool;      // 512 voxel ids per occupied brick, voxel (x,y,z) of the brick at x + 8y + 64z
    const uint8_t*  bfine;      // per occupied brick 8 octants x 512 voxels: 0 = solid, else min(16, side of the largest empty cube
                                // of VOXELS cornered here ...), looking through the brick's 26 neighbours
    int32_t         pbx, pby;
    const uint64_t* bentry;     // what a look-up of the march reads: ONE 8-byte word per brick of the padded grid (brick_entry_pack):
                                // bits 0..23 the pointer (0 empty, 0xFFFFFF border, else 1 + pool index), bits 24..31 "open" per octant,
                                // bits 32..63 the coarse clearance of the eight octants, four bits each (0 = occupied or border, else
                                // min(15, bricks)) -- bgrid and bcoarse folded into one load instead of two dependent ones
    uint32_t        df_own;      // 1: AO rays through df_any_loop (development switch)
    uint32_t        ao_batch;    // 1: the hand-written loop's kernels trace the AO rays of a wave from a pool in LDS every lane draws on (df_ao_pool_loop; context option "ao_batch")
    uint32_t        df_prefetch; // 1: the secondary rays' look-ups through trace_df_fast prefetch the neighbouring rows (development switch)
    uint32_t        df_thresh;   // 1: primary rays through df_prim_loop (long runs by threshold; launches that report no iteration counts)
    uint32_t        brick_open;  // 1: bit 7 of a coarse byte (no occupied brick is left in the box between this brick and the volume's
                                // corner in the octant's direction: a ray here is a miss) ends the march; 0: the bit is ignored   // padded grid dimensions in x and y
    int32_t W, H, D;
    int32_t n1x, n1y, n1z;
    int32_t n2x, n2y, n2z;
    int32_t n3x, n3y, n3z;
};

struct RayInt {            // RayHitInternal, voxel_volume.frag:33-41
    f3 pos, side, delta;
    int sx, sy, sz;        // rayStep
    int mx, my, mz;        // mapPos at loop exit
    uint32_t material;
    uint32_t mask;         // bit0..2
    uint32_t fetches;      // DENSE/BITMASK: iterations that sampled a voxel (frag:157); JUMP: upper bound
    uint32_t dbg0, dbg1;   // traversal diagnostics (outer iterations / near-regime iterations of trace_skip)
};

struct TraceStats {        // host-side instrumentation (tests); a no-op type is used on the device
    uint32_t literal = 0, jumps1 = 0, jumps2 = 0, jumps3 = 0, retrace = 0, lookups = 0;
};
struct NoStats {};
VRT_HD void st_literal(TraceStats& s) { s.literal++; }
VRT_HD void st_jump(TraceStats& s, int lvl) { if (lvl == 1) s.jumps1++; else if (lvl == 2) s.jumps2++; else s.jumps3++; }
VRT_HD void st_retrace(TraceStats& s) { s.retrace++; }
VRT_HD void st_lookup(TraceStats& s) { s.lookups++; }
VRT_HD void st_literal(NoStats&) {}
VRT_HD void st_jump(NoStats&, int) {}
VRT_HD void st_retrace(NoStats&) {}
VRT_HD void st_lookup(NoStats&) {}

VRT_HD uint32_t f2u(float f)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_uint(f);
#else
    union { float f; uint32_t u; } c; c.f = f; return c.u;
#endif
}
VRT_HD float u2f(uint32_t u)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(u);
#else
    union { float f; uint32_t u; } c; c.u = u; return c.f;
#endif
}
VRT_HD float rcp_approx(float x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_rcpf(x);
#else
    return 1.0f / x;
#endif
}

// ---- occupancy lookups ------------------------------------------------------------------------------

VRT_HD uint32_t cell_bit(int x, int y, int z) { return (uint32_t)(x & 3) | ((uint32_t)(y & 3) << 2) | ((uint32_t)(z & 3) << 4); }

// occ1 word of 4^3 cell (cx,cy,cz); the 16^3 summary is consulted first so empty space costs no global access.
template <class OP>
VRT_HD uint64_t fetch_cell(const VolumeView& v, OP o2, int cx, int cy, int cz)
{
    uint64_t w2 = o2[(cx >> 2) + ((cy >> 2) + (cz >> 2) * v.n2y) * v.n2x];
    if (!((w2 >> cell_bit(cx, cy, cz)) & 1ull)) return 0ull;
    return v.occ1[cx + (cy + cz * v.n1y) * v.n1x];
}

// Emptiness level of the pyramid at voxel (mx,my,mz): 3 = its 64^3 cell is empty, 2 = its 16^3 cell, 1 = its
// 4^3 cell, 0 = the 4^3 cell holds voxels (word = its occ1 bits).
template <class OP>
VRT_HD int lookup_level(const VolumeView& v, OP o2, OP o3, int mx, int my, int mz, uint64_t& word)
{
    int cx = mx >> 2, cy = my >> 2, cz = mz >> 2;
    int qx = cx >> 2, qy = cy >> 2, qz = cz >> 2;
    uint64_t w3 = o3[(qx >> 2) + ((qy >> 2) + (qz >> 2) * v.n3y) * v.n3x];
    word = 0ull;
    if (w3 == 0ull) return 3;
    if (!((w3 >> cell_bit(qx, qy, qz)) & 1ull)) return 2;
    uint64_t w2 = o2[qx + (qy + qz * v.n2y) * v.n2x];
    if (!((w2 >> cell_bit(cx, cy, cz)) & 1ull)) return 1;
    word = v.occ1[cx + (cy + cz * v.n1y) * v.n1x];
    return 0;
}

// Each clearance field is a plain x-fastest volume with a one-voxel border of zeros on every side, (W+2)(H+2)(D+2)
// bytes: voxel (x,y,z) lives at (x+1) + (y+1)*(W+2) + (z+1)*(W+2)*(H+2).  A run can carry a ray at most one voxel
// past a wall (the fields count the outside as solid), so the traversal may read the field wherever a run ends
// without a bounds test, and it keeps the index incrementally (two 24-bit multiply-adds per look-up).  An earlier
// layout in 4x4x4 bricks touched fewer cache lines per gather but cost 12 VALU ops of index arithmetic plus the
// bounds test per look-up; the kernel is bound by VALU issue, not by the vector-memory pipe.
VRT_HD size_t df_index(const VolumeView& v, int x, int y, int z)
{
    const size_t pw = (size_t)v.W + 2u, ph = (size_t)v.H + 2u;
    return (size_t)(x + 1) + ((size_t)(y + 1) + (size_t)(z + 1) * ph) * pw;
}
VRT_HD size_t df_field_bytes(int W, int H, int D)            // one padded field, rounded up to 256 B
{
    size_t n = ((size_t)W + 2u) * ((size_t)H + 2u) * ((size_t)D + 2u);
    return (n + 255u) & ~(size_t)255u;
}
// 32-bit incremental indexing: all eight fields below 4 GiB and a padded z-slice that fits a signed 24-bit multiply
VRT_HD bool df_small(const VolumeView& v)
{
    return 8ull * v.df_stride <= 0xFFFFFFFFull && ((uint64_t)v.W + 2u) * ((uint64_t)v.H + 2u) < (1ull << 23);
}
// trace_df_fast's layout (nine fields + the 0xFF byte, every offset 32 bits): the loop counts its offsets from `bias` =
// (W+2)(H+2) bytes IN FRONT of field 0, so the largest offset it forms is bias + 9 * field (the 0xFF byte), a hit's id read
// reaches bias + 8 * field + index, and a live lane's prefetch one slice (bias bytes) past its own index -- all of it must
// stay below 2^32, and the padded slice must fit the signed 24-bit multiply of the index recovery.
VRT_HD bool df_fast_layout_ok(int W, int H, int D)
{
    const uint64_t pwh = ((uint64_t)W + 2u) * ((uint64_t)H + 2u);
    return 2ull * pwh + 9ull * (uint64_t)df_field_bytes(W, H, D) + 256ull <= 0xFFFFFFFFull && pwh < (1ull << 23);
}
template <bool SMALL> struct IndexT;
template <> struct IndexT<true>  { typedef uint32_t type; typedef int32_t stype; };
template <> struct IndexT<false> { typedef size_t type;   typedef long long stype; };
// a * b for |a|, |b| < 2^23 (one v_mul_i32_i24 / v_mad_i32_i24 instead of the quarter-rate 32-bit multiply)
VRT_HD int mul24(int a, int b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __mul24(a, b);
#else
    return a * b;
#endif
}

VRT_HD bool oob(const VolumeView& v, int mx, int my, int mz)
{
    return (uint32_t)mx >= (uint32_t)v.W || (uint32_t)my >= (uint32_t)v.H || (uint32_t)mz >= (uint32_t)v.D;
}

VRT_HD uint32_t voxel_at(const VolumeView& v, int mx, int my, int mz)
{
    return v.vox[(size_t)mx + ((size_t)my + (size_t)mz * (size_t)v.H) * (size_t)v.W];
}

VRT_HD uint32_t umin3(uint32_t a, uint32_t b, uint32_t c) { uint32_t m = a < b ? a : b; return m < c ? m : c; }

// the one 8-byte word per brick of the padded grid that a look-up of the brick march reads (VolumeView::bentry)
VRT_HD uint64_t brick_entry_pack(uint32_t ptr, const uint8_t coarse[8])
{
    // ptr: a padded-grid entry (0 empty, 0xFFFFFFFF border, else 1 + pool index < 0xFFFFFF); coarse[o]: the octant's coarse byte
    // (low 7 bits: clearance in bricks, 0 = occupied or border; bit 7: open).  A clearance above 15 is stored as 15: any
    // lower bound of the true clearance gives the same march.
    uint32_t lo = ptr == 0xFFFFFFFFu ? 0xFFFFFFu : (ptr & 0xFFFFFFu), hi = 0u;
    for (int o = 0; o < 8; o++) {
        const uint32_t c = coarse[o] & 0x7Fu;
        hi |= (c > 15u ? 15u : c) << (4 * o);
        if (coarse[o] & 0x80u) lo |= 1u << (24 + o);
    }
    return (uint64_t)lo | ((uint64_t)hi << 32);
}

} // namespace vrt
