// vrt_frame_slot.h -- how a workgroup of the render stage finds its work and its outputs, device only: the frame slot of a
// launch read from the kernel arguments or from the table (SlotOf<>, table_read, kernarg_words, MissPlanes), pointers into
// global memory by 32-bit offset (gptr), the workgroup -> tile map (udiv_uniform, block_to_tile, tile_origin), the occupancy
// summaries as a workgroup sees them (OccT, stage_occ) and the colour store (store_color).  Used by K1, K2 and k_tile_tags.
// kernarg_words and SlotOf<false> read the kernel-argument segment and are valid ONLY in a kernel whose sole argument is
// GeomParams; the shading path (vrt_shade.h) uses neither.
#pragma once

#include "vrt_device_common.h"

namespace vrt {

// ---------------------------------------------------------------------------------------------
// tile mapping
// ---------------------------------------------------------------------------------------------

// Workgroup -> screen tile.  Workgroups are dealt round-robin over the 8 XCDs (b and b+8 share an
// XCD and its private 4 MiB L2), so XCD slot (b % 8) gets one contiguous run of `chunk` tiles in
// row-major tile order: neighbouring tiles traverse neighbouring volume cells and share L2 lines.
// n / d for wave-uniform operands with rcp = floor(2^32 / d): mulhi is the quotient or one below it, one correction
// step makes it exact for every n < 2^32.  Stays on the scalar unit (a generic 32-bit division is ~20 VALU ops).
__device__ __forceinline__ uint32_t udiv_uniform(uint32_t n, uint32_t d, uint32_t rcp, uint32_t& rem)
{
    uint32_t q = (uint32_t)(((uint64_t)n * (uint64_t)rcp) >> 32);
    uint32_t r = n - q * d;
    if (r >= d) { q++; r -= d; }
    rem = r;
    return q;
}

// The slot (camera, planes, strip assignment) of frame `frame` of the launch.  TABLE = false: a reference into the kernel
// arguments.  TABLE = true (launches of more than VRT_MAX_BATCH frames): a copy read from the table in device memory
// through the constant address space -- the table is not written while the kernel runs, and only loads the compiler
// knows to be invariant become scalar loads (a plain global pointer gives vector loads and the slot in VGPRs).
typedef const __attribute__((address_space(4))) uint32_t* const_u32_ptr;
// n dwords starting at byte offset `off` of slot `frame` of the table, read through the constant address space
template <int N> __device__ __forceinline__ void table_read(const GeomParams& P, uint32_t frame, size_t off, void* dst)
{
    const_u32_ptr w = (const_u32_ptr)((const char*)(P.table + frame) + off);
    uint32_t tmp[N];
#pragma unroll
    for (int i = 0; i < N; i++) tmp[i] = w[i];
    __builtin_memcpy(dst, tmp, sizeof tmp);
}
// The kernel's own arguments (GeomParams is the one argument, at offset 0 of the segment) as words to be read NOW: the
// compiler hoists ordinary argument loads to the top of the kernel, where each costs scalar registers across ray generation;
// what only a rare or late branch needs is read through this pointer, which it cannot see through.
// VALID ONLY in a kernel whose sole argument is GeomParams (k_primary, k_tile_tags): byte_offset is an offsetof(GeomParams, ...)
// applied to the segment of whatever kernel runs, and in any other kernel it reads that kernel's arguments as if they were
// GeomParams -- pointers assembled from those words fault.  (Conservative: what the code needs is GeomParams at offset 0 of the
// segment, which k_hit_colors' (GeomParams, uint32_t*) would satisfy too; it calls none of this.)  So is everything that calls it: SlotOf<false>::cam_pos, ::ptrs and
// ::miss_planes, and K1's own reads of sky8 / skyk and of the tile map's flags.
__device__ __forceinline__ const_u32_ptr kernarg_words(size_t byte_offset)
{
    const_u32_ptr p = (const_u32_ptr)((const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr() + byte_offset);
    asm volatile("" : "+s"(p));
    return p;
}
// base + 32-bit byte offset as a pointer into GLOBAL memory (address space 1): global_load / global_store with the base in a
// scalar pair and the offset in one vector register
template <class T> __device__ __forceinline__ __attribute__((address_space(1))) T* gptr(const void* base, uint32_t byte_offset)
{
    return (__attribute__((address_space(1))) T*)((__attribute__((address_space(1))) char*)base + byte_offset);
}
typedef float vrt_f4 __attribute__((ext_vector_type(4)));
typedef float vrt_f2 __attribute__((ext_vector_type(2)));
// the planes a miss pixel is stored to (the fast sky wave reads these eight pointers, not all fourteen)
struct MissPlanes { uint8_t* color8; float* depth; float* motion; uint8_t* mask8; float* position; int8_t* normal8; uint8_t* hit_id; uint8_t* color8_strips; };
template <bool TABLE> struct SlotOf;
template <> struct SlotOf<false> {
    static __device__ __forceinline__ void head(const GeomParams& P, uint32_t frame, RayGenConsts& g, float* cam_right, int& shard_rank, uint32_t& box)
    {
        const FrameSlot& S = P.slot[frame];
        box = (uint32_t)S.box[0] | ((uint32_t)S.box[1] << 8) | ((uint32_t)S.box[2] << 16) | ((uint32_t)S.box[3] << 24);
        g = S.rg;
        cam_right[0] = S.pc.cam_right[0]; cam_right[1] = S.pc.cam_right[1]; cam_right[2] = S.pc.cam_right[2];
        shard_rank = S.shard_rank;
    }
    static __device__ __forceinline__ vrt_frame planes(const GeomParams& P, uint32_t frame) { return P.slot[frame].fr; }
    // the camera position: only waves that trace need it, and they read it when they know they do (three scalar registers
    // less across ray generation for everybody)
    static __device__ __forceinline__ f3 cam_pos(const GeomParams& P, uint32_t frame)
    {
        const_u32_ptr w = kernarg_words(offsetof(GeomParams, slot) + (size_t)frame * sizeof(FrameSlot) + offsetof(FrameSlot, pc) + offsetof(vrt_push, cam_pos));
        return mk3(__uint_as_float(w[0]), __uint_as_float(w[1]), __uint_as_float(w[2]));
    }
    // N plane pointers of the frame starting with field `first` of vrt_frame, read NOW (kernarg_words)
    template <int N> static __device__ __forceinline__ void ptrs(const GeomParams& P, uint32_t frame, int first, void** out)
    {
        const_u32_ptr fp = kernarg_words(offsetof(GeomParams, slot) + (size_t)frame * sizeof(FrameSlot) + offsetof(FrameSlot, fr) + 8u * (size_t)first);
        uint32_t tmp[2 * N];
#pragma unroll
        for (int q = 0; q < 2 * N; q++) tmp[q] = fp[q];
        __builtin_memcpy(out, tmp, sizeof tmp);
    }
    static __device__ __forceinline__ MissPlanes miss_planes(const GeomParams& P, uint32_t frame)
    {
        // (read late, like the fast path's other constants: through a pointer into the arguments the compiler cannot hoist from)
        // words 0 - 11 of vrt_frame are color8 .. normal8, 14 - 15 hit_id, 26 - 27 color8_strips, and MissPlanes is those eight pointers
        static_assert(offsetof(vrt_frame, color8) == 0 && offsetof(vrt_frame, normal8) == 40 && offsetof(vrt_frame, hit_id) == 56 &&
                      offsetof(vrt_frame, color8_strips) == 104 && sizeof(MissPlanes) == 64, "vrt_frame layout");
        const_u32_ptr fp = kernarg_words(offsetof(GeomParams, slot) + (size_t)frame * sizeof(FrameSlot) + offsetof(FrameSlot, fr));
        MissPlanes m;
        uint32_t tmp[16];
#pragma unroll
        for (int q = 0; q < 12; q++) tmp[q] = fp[q];
        tmp[12] = fp[14]; tmp[13] = fp[15]; tmp[14] = fp[26]; tmp[15] = fp[27];
        __builtin_memcpy(&m, tmp, sizeof m);
        return m;
    }
    static __device__ __forceinline__ const vrt_push* push(const GeomParams& P, uint32_t frame) { return &P.slot[frame].pc; }
};
// The table form reads the pieces when they are needed, like the kernel-argument form does: a copy of the whole slot at the
// top keeps the fourteen plane pointers in scalar registers through the traversal (82 + 6 SGPRs: one wave per SIMD less).
template <> struct SlotOf<true> {
    static __device__ __forceinline__ void head(const GeomParams& P, uint32_t frame, RayGenConsts& g, float* cam_right, int& shard_rank, uint32_t& box)
    {
        table_read<1>(P, frame, offsetof(FrameSlot, box), &box);
        table_read<sizeof(RayGenConsts) / 4>(P, frame, offsetof(FrameSlot, rg), &g);
        table_read<3>(P, frame, offsetof(FrameSlot, pc) + offsetof(vrt_push, cam_right), cam_right);
        table_read<1>(P, frame, offsetof(FrameSlot, shard_rank), &shard_rank);
    }
    // the head without the box word: a kernel that reads its block's verdict (GeomParams::verdicts; table launches only) has no
    // use for the rectangle
    static __device__ __forceinline__ void head_no_box(const GeomParams& P, uint32_t frame, RayGenConsts& g, float* cam_right, int& shard_rank)
    {
        table_read<sizeof(RayGenConsts) / 4>(P, frame, offsetof(FrameSlot, rg), &g);
        table_read<3>(P, frame, offsetof(FrameSlot, pc) + offsetof(vrt_push, cam_right), cam_right);
        table_read<1>(P, frame, offsetof(FrameSlot, shard_rank), &shard_rank);
    }
    // the strip assignment and the box word alone (k_block_verdicts)
    static __device__ __forceinline__ void rank_box(const GeomParams& P, uint32_t frame, int& shard_rank, uint32_t& box)
    {
        table_read<1>(P, frame, offsetof(FrameSlot, shard_rank), &shard_rank);
        table_read<1>(P, frame, offsetof(FrameSlot, box), &box);
    }
    static __device__ __forceinline__ vrt_frame planes(const GeomParams& P, uint32_t frame)
    {
        vrt_frame f;
        table_read<sizeof(vrt_frame) / 4>(P, frame, offsetof(FrameSlot, fr), &f);
        return f;
    }
    static __device__ __forceinline__ f3 cam_pos(const GeomParams& P, uint32_t frame)
    {
        const_u32_ptr w = (const_u32_ptr)((const char*)(P.table + frame) + offsetof(FrameSlot, pc) + offsetof(vrt_push, cam_pos));
        asm volatile("" : "+s"(w));
        return mk3(__uint_as_float(w[0]), __uint_as_float(w[1]), __uint_as_float(w[2]));
    }
    template <int N> static __device__ __forceinline__ void ptrs(const GeomParams& P, uint32_t frame, int first, void** out)
    {
        const_u32_ptr w = (const_u32_ptr)((const char*)(P.table + frame) + offsetof(FrameSlot, fr) + 8u * (size_t)first);
        asm volatile("" : "+s"(w));                            // (read NOW: not hoisted to where the slot's head is read)
        uint32_t tmp[2 * N];
#pragma unroll
        for (int q = 0; q < 2 * N; q++) tmp[q] = w[q];
        __builtin_memcpy(out, tmp, sizeof tmp);
    }
    static __device__ __forceinline__ MissPlanes miss_planes(const GeomParams& P, uint32_t frame)
    {
        // color8 .. normal8 are the first six pointers of vrt_frame, hit_id the eighth, color8_strips the fourteenth
        static_assert(offsetof(vrt_frame, normal8) == 40 && offsetof(vrt_frame, hit_id) == 56 && offsetof(vrt_frame, color8_strips) == 104, "vrt_frame layout");
        MissPlanes m;
        table_read<12>(P, frame, offsetof(FrameSlot, fr), &m);
        table_read<2>(P, frame, offsetof(FrameSlot, fr) + offsetof(vrt_frame, hit_id), &m.hit_id);
        table_read<2>(P, frame, offsetof(FrameSlot, fr) + offsetof(vrt_frame, color8_strips), &m.color8_strips);
        return m;
    }
    static __device__ __forceinline__ const vrt_push* push(const GeomParams& P, uint32_t frame) { return &P.table[frame].pc; }
};

// workgroup -> frame of the launch and tile row within the frame's local rows (ty) and tile column (tx).  Frames of a
// batch follow one another in the grid: the next frame's first tiles start while this one drains.
// XCD x (= workgroup id & 7) owns every 8th tile row: every XCD gets an even sample of sky and geometry (a contiguous
// band per XCD leaves the XCDs that drew the sky idle), while the tiles of one row -- which walk neighbouring volume cells
// -- still share that XCD's L2.
//   xcd_turn == 0: per frame, row ty belongs to XCD ty % 8; ceil(rows / 8) * 8 row slots per frame (the surplus
//                  workgroups exit at once).
//   xcd_turn == 1: the rows of ALL frames of the launch are dealt round-robin in one sequence (row L = frame * rows + ty
//                  to XCD L % 8).  For row counts far from a multiple of 8 -- a rank's 18 rows of a sharded 1080p frame
//                  would be 3 rows for two XCDs and 2 for the others, and a third of the grid would be surplus -- the XCDs
//                  stay even and only the last seven row slots of the launch can be empty.
// MAP: the launch's xcd_turn as a compile-time constant (the product traversals), or -1: looked at here
template <int MAP>
__device__ __forceinline__ bool block_to_tile(const TileMap& M, uint32_t& frame, int& ty, int& tx)
{
    // xcd_turn 0 and 2 are launched as THREE-dimensional grids (8 x columns, rows, frames): the workgroup's three indices are in
    // scalar registers when the wave starts, and the XCD (workgroups are dealt to the eight XCDs in dispatch order, x fastest)
    // is the low three bits of the x index because the grid's x extent is a multiple of 8 -- no division, where the linear
    // form spends two or three (ten scalar instructions each, in a kernel whose scalar unit -- ONE per CU, shared by its four
    // SIMDs -- is as busy as its vector units: a 1080p frame of sky-only waves that return once they know their block takes
    // 11 us, 158 scalar instructions per wave).
    if (MAP == 2 || (MAP < 0 && M.xcd_turn == 2)) {
        // per frame every XCD owns ONE of 8 screen regions (2 columns x 4 rows of tiles), and the assignment rotates from frame
        // to frame (XCD x traces region (x + frame) % 8): an XCD's rays of one frame then walk one eighth of the volume in one
        // or two direction octants -- a working set of clearance bytes that fits its 4 MiB L2 instead of the whole 17 MB field
        // -- while over 8 frames every XCD traces every region once, so sky and geometry regions balance.
        const uint32_t rw = ((uint32_t)M.tiles_x + 1u) >> 1, rh = ((uint32_t)M.tiles_y_local + 3u) >> 2;
        frame = blockIdx.z;
        const uint32_t region = ((blockIdx.x & 7u) + frame) & 7u;
        tx = (int)((blockIdx.x >> 3) + (region & 1u) * rw);
        ty = (int)(blockIdx.y + (region >> 1) * rh);
        return tx < M.tiles_x && ty < M.tiles_y_local;
    }
    if (MAP == 0 || (MAP < 0 && M.xcd_turn == 0)) {
        // per frame, row ty belongs to XCD ty % 8: every XCD gets an even sample of sky and geometry (a contiguous band per XCD
        // leaves the XCDs that drew the sky idle), while the tiles of one row -- which walk neighbouring volume cells -- still
        // share that XCD's L2; ceil(rows / 8) * 8 row slots per frame (the surplus workgroups exit at once)
        frame = blockIdx.z;
        tx = (int)(blockIdx.x >> 3);
        ty = (int)(blockIdx.y * 8u + (blockIdx.x & 7u));
        return ty < M.tiles_y_local;
    }
    // xcd_turn == 1 (a one-dimensional grid): the rows of ALL frames of the launch are dealt round-robin in one sequence (row
    // L = frame * rows + ty to XCD L % 8).  For row counts far from a multiple of 8 -- a rank's 18 rows of a sharded 1080p
    // frame would be 3 rows for two XCDs and 2 for the others, and a third of the grid would be surplus -- the XCDs stay even
    // and only the last seven row slots of the launch can be empty.
    uint32_t b = blockIdx.x, utx, uty;
    uint32_t L = udiv_uniform(b >> 3, (uint32_t)M.tiles_x, M.tiles_x_rcp, utx) * 8u + (b & 7u);
    frame = udiv_uniform(L, (uint32_t)M.tiles_y_local, M.tiles_y_rcp, uty);
    ty = (int)uty; tx = (int)utx;
    return frame < (uint32_t)M.n_frames;
}

// yp0: the row of y0 in the rank's packed strips (vrt_pack_rows order)
__device__ __forceinline__ bool tile_origin(const TileMap& M, int ty, int tx, int shard_rank, int& x0, int& y0, int& yp0)
{
    // bottom rows first: the rows dispatched last only have the drain of the machine to hide in, and the top of a
    // frame is where the cheap sky-only tiles usually are
    ty = M.tiles_y_local - 1 - ty;
    uint32_t within = (uint32_t)ty;
    int strip_local = 0;                                       // (unsharded: the frame is one strip)
    if (M.nranks > 1) strip_local = (int)udiv_uniform((uint32_t)ty, M.tps, M.tps_rcp, within);
    x0 = tx * M.tile;
    yp0 = strip_local * M.strip_rows + (int)within * M.tile;
    y0 = (strip_local * M.nranks + shard_rank) * M.strip_rows + (int)within * M.tile;
    return y0 < M.H;
}

// Occupancy summaries as seen by a workgroup: LDS copies when they fit (typed address_space(3) pointers, so
// that the lookups compile to ds_read_b64 and not to flat loads), the L2-resident originals otherwise.
typedef const __attribute__((address_space(3))) uint64_t* lds_u64_ptr;
template <bool LDS> struct OccT;
template <> struct OccT<true>  { lds_u64_ptr o2, o3; };
template <> struct OccT<false> { const uint64_t* o2; const uint64_t* o3; };

// Stage the 16^3 and 64^3 occupancy summaries into LDS (16 B per lane per iteration, coalesced).
template <bool LDS> __device__ __forceinline__ OccT<LDS> stage_occ(const GeomParams& P, uint64_t* lds);
template <> __device__ __forceinline__ OccT<false> stage_occ<false>(const GeomParams& P, uint64_t*)
{
    OccT<false> o; o.o2 = P.sc.vol.occ2; o.o3 = P.sc.vol.occ3; return o;
}
template <> __device__ __forceinline__ OccT<true> stage_occ<true>(const GeomParams& P, uint64_t* lds)
{
    const uint4* src2 = reinterpret_cast<const uint4*>(P.sc.vol.occ2);
    const uint4* src3 = reinterpret_cast<const uint4*>(P.sc.vol.occ3);
    uint4* dst = reinterpret_cast<uint4*>(lds);
    uint32_t n2 = P.occ2_bytes / 16, n3 = P.occ3_bytes / 16;
    for (uint32_t i = threadIdx.x; i < n2; i += blockDim.x) dst[i] = src2[i];
    for (uint32_t i = threadIdx.x; i < n3; i += blockDim.x) dst[n2 + i] = src3[i];
    __syncthreads();
    OccT<true> o;
    o.o2 = (lds_u64_ptr)lds; o.o3 = (lds_u64_ptr)(lds + P.occ2_bytes / 8);
    return o;
}

// the pixel's colour into color_f (debug), color8 and the packed strips
__device__ __forceinline__ void store_color(const vrt_frame& f, f3 col, size_t i, uint32_t i32, uint32_t strip_off)
{
    if (f.color_f) { f.color_f[i * 3 + 0] = col.x; f.color_f[i * 3 + 1] = col.y; f.color_f[i * 3 + 2] = col.z; }
    if (f.color8 || f.color8_strips) {
        const uint32_t c8 = (uint32_t)unorm8(col.x) | ((uint32_t)unorm8(col.y) << 8) | ((uint32_t)unorm8(col.z) << 16);
        if (f.color8) *gptr<uint32_t>(f.color8, i32 << 2) = c8;
        if (f.color8_strips) *gptr<uint32_t>(f.color8_strips, strip_off) = c8;
    }
}

} // namespace vrt
