// vrt_device.hip -- the render stage: hand-written HIP kernels for gfx950 (MI355X, CDNA4; 64-wide wavefronts).
//
//   k_primary<...>    K1: per-pixel ray generation + Amanatides-Woo DDA + G-buffer write
//                     (voxel_volume.frag:309-346, :109-196 of the reference)
//   k_shade<...>      K2: AO / shadow / mirror-bounce rays + shading (voxel_volume.frag:205-307)
//   k_sky_*, k_hit_colors, k_tile_tags   the tables and tags K1 reads
// (scene build: vrt_scene_build.hip; scene edits: vrt_scene_edit.hip; K3: vrt_denoise.hip; strips, blit, accumulate, resolve:
// vrt_post.hip.)  Compiled in four parts, -DVRT_K1_PART=0..3: the list behind launch_shade_t.
// This file is the kernels and their launch code.  What they are made of: vrt_shade.h (traceRay, the secondary rays, colorHit,
// colorMainRay -- and, at its head, what a kernel that calls them owes them), vrt_frame_slot.h (the frame slot from the kernel
// arguments or the table, the workgroup -> tile map, the colour store), vrt_traverse.h (the dispatch over the marches, vrt_march_*.h).
//
// A wave owns an 8x8 pixel block so that its 64 rays stay spatially coherent; the default (clearance-field)
// traversal runs one wave per workgroup, the LDS-staged ones 16x16 tiles of four waves.  Rays are generated in-kernel
// from the 96-byte push-constant block (no ray buffers); a launch covers up to 8 frames.  No MFMA: nothing here is a
// dense contraction.
//
// All arithmetic follows vrt_spec.h (fp32, -ffp-contract=off); the DDA state (sideDist, mapPos, mask)
// is advanced with exactly the additions of voxel_volume.frag:164-170 in every traversal mode, so hit
// voxel, mask, t and step budget are independent of the mode.
#include "vrt_shade.h"
#include "vrt_frame_slot.h"

namespace vrt {

// ---------------------------------------------------------------------------------------------
// K1: primary rays
// ---------------------------------------------------------------------------------------------

// What a sky wave with a miss-colour plane stores for its pixel: zeros in every plane but the colour's, c8 there -- the stores of
// k_primary's short path, statement for statement (kept there as they are: moved into this function, every kernel's machine code
// changes).  flags: the tile map's; span_nt: the wave holds two whole rows of an all-sky span (vrt_span.h), whose planes of zeros go
// out as non-temporal stores; strip_off: the pixel's byte offset in the rank's packed strips.
__device__ __forceinline__ void store_miss_pixel(const MissPlanes& f, uint32_t flags, bool span_nt, uint32_t i32, uint32_t c8, uint32_t strip_off)
{
    if (span_nt && (flags & VRT_MAPFLAG_SIX)) {
        __builtin_nontemporal_store((vrt_f4){0.0f, 0.0f, 0.0f, 0.0f}, gptr<vrt_f4>(f.position, i32 << 4));
        __builtin_nontemporal_store((vrt_f2){0.0f, 0.0f}, gptr<vrt_f2>(f.motion, i32 << 3));
        __builtin_nontemporal_store(0.0f, gptr<float>(f.depth, i32 << 2));
        __builtin_nontemporal_store(0u, gptr<uint32_t>(f.normal8, i32 << 2));
        __builtin_nontemporal_store((uint8_t)0, gptr<uint8_t>(f.mask8, i32));
        *gptr<uint32_t>(f.color8, i32 << 2) = c8;
        return;
    }
    if (flags & VRT_MAPFLAG_SIX) {                       // the reference's six targets and nothing else: six stores, no pointer tested
        *gptr<vrt_f4>(f.position, i32 << 4) = (vrt_f4){0.0f, 0.0f, 0.0f, 0.0f};
        *gptr<vrt_f2>(f.motion, i32 << 3) = (vrt_f2){0.0f, 0.0f};
        *gptr<float>(f.depth, i32 << 2) = 0.0f;
        *gptr<uint32_t>(f.normal8, i32 << 2) = 0u;
        *gptr<uint8_t>(f.mask8, i32) = (uint8_t)0;
        *gptr<uint32_t>(f.color8, i32 << 2) = c8;
        return;
    }
    if (f.position) *gptr<vrt_f4>(f.position, i32 << 4) = (vrt_f4){0.0f, 0.0f, 0.0f, 0.0f};
    if (f.motion) *gptr<vrt_f2>(f.motion, i32 << 3) = (vrt_f2){0.0f, 0.0f};
    if (f.depth) *gptr<float>(f.depth, i32 << 2) = 0.0f;
    if (f.normal8) *gptr<uint32_t>(f.normal8, i32 << 2) = 0u;
    if (f.mask8) *gptr<uint8_t>(f.mask8, i32) = (uint8_t)0;
    if (f.hit_id) *gptr<uint8_t>(f.hit_id, i32) = (uint8_t)0;
    if (f.color8) *gptr<uint32_t>(f.color8, i32 << 2) = c8;
    if (f.color8_strips) *gptr<uint32_t>(f.color8_strips, strip_off) = c8;
}

// MODE 0: write hit records for K2 (split);  1: no secondary rays enabled, shade inline;  4: the megakernel without its bounce loop;
// MODE 5, 6, 7: the megakernel with the bounce chain as one word per hit (color_main_ray_packed: no stack of hits; what the product
//         traversals launch) for at most 2 / 5 / VRT_MAX_BOUNCES bounces;
// MODE 2: megakernel -- the lanes that hit go on to trace their AO / shadow / bounce rays in this same kernel, so that
//         the secondary rays' latency hides under the primary work of the other waves (a separate K2 launch has a
//         single round of waves and is bound by the longest ray's dependency chain).
// At least 7 waves per SIMD for every MODE: the packed-chain megakernels measured 1 075 us at 7 (72 VGPRs, spilling), 1 148 at 6 and 1 165 at 5
// (Mandelbulb 4K); forcing the megakernel without its bounce loop to 8 (64 VGPRs) costs 12 B of scratch per lane.
template <int TRAV, bool OCC_LDS, int MODE, bool TABLE, int MAP>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(7, 8))) void k_primary(const GeomParams P)
{
    extern __shared__ __attribute__((aligned(16))) uint64_t lds_occ[];
    // the tile map arrives with one 64-byte scalar load (and one wait) before anything depends on it
    TileMap M = P.map;
    const uint64_t t_begin = (M.flags & 2u) ? wall_clock64() : 0ull;         // diagnostic timeline (100 MHz)
    int x0, y0, yp0, ty, tx;
    uint32_t frame;
    if (!block_to_tile<MAP>(M, frame, ty, tx)) return;                   // uniform per workgroup
    // the block's tile tag (k_tile_tags) and the frame's "the tags say nothing" word: two scalar loads that leave together with
    // the frame slot's (their address needs nothing from the slot: tags are laid out in the launch's LOCAL rows of 8x8 blocks,
    // in dispatch order), looked at after ray generation.  Written by the kernel before this one: constant address space.
    // (A launch without tags points at one word per frame that holds its tile_gen, with tags_x = 0 and tags_per_frame = 1.)
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t tile_gen = P.tile_gen;
    // (vrt_span.h: with them leave the four tags of the block's 32x8 span -- neighbours in one tag row.  The primary-only kernels
    // fetch them with ONE four-word load at the span's first block whatever the launch: a cut span and a launch without tags look
    // at their own word of the four only.  The megakernels keep the four single loads -- the block's own four times over where
    // the span is cut or the launch has no span path, the frame's one word without tags: with the short form their packed bounce
    // chains spill a register more, 168 / 196 B per lane against budgets of 160 / 192, tools/check_resources.py)
    // (vrt_span.h block_verdict_byte: the primary-only kernels of TABLE launches fetch neither -- k_block_verdicts, launched behind
    // k_tile_tags, has looked at the tags, the frame's word and the box rectangle for every block of the launch, and the wave reads
    // the ONE word that holds its span's four bytes, with one scalar load that leaves with the slot's.  Launches with their slots
    // in the kernel arguments -- eight frames at most, one in a frame loop -- keep the one-fetch form: there a kernel more ahead of
    // K1 costs more than the shorter preamble of so few waves returns)
    constexpr bool kVerdict = MODE == 1 && TABLE;
    constexpr bool kOneFetch = MODE == 1 && !kVerdict;
    typedef uint32_t span_words __attribute__((ext_vector_type(4), aligned(4)));
    span_words st;
    uint32_t tag_all = 0u, own = 0u, tag = 0u, vword = 0u, role = 0u;
    bool span_w = false, wide = false;
    if constexpr (kVerdict) {
        const uint32_t sh = (uint32_t)M.tile >> 4;
        const uint32_t row8 = ((uint32_t)ty << sh) + (uint32_t)(wave >> 1), col8 = ((uint32_t)tx << sh) + (uint32_t)(wave & 1);
        role = span_role(col8);
        const uint32_t pitch = verdict_pitch((uint32_t)M.tiles_x << sh);
        vword = *(const_u32_ptr)((const __attribute__((address_space(4))) char*)P.verdicts + verdict_word(row8, col8, frame, (uint32_t)M.n_frames, pitch));
    } else {
        const_u32_ptr tg = (const_u32_ptr)(P.tile_tags + (size_t)frame * P.tags_per_frame);
        const uint32_t tags_x = P.tags_x, sh = (uint32_t)M.tile >> 4;
        const uint32_t row8 = ((uint32_t)ty << sh) + (uint32_t)(wave >> 1), col8 = ((uint32_t)tx << sh) + (uint32_t)(wave & 1);
        span_w = (M.flags & VRT_MAPFLAG_SKY_SPAN) != 0u && span_in_frame(span_x0(col8), (uint32_t)M.W);
        wide = span_w && tags_x != 0u;
        if (kOneFetch) {
            own = span_fetch_own(col8, tags_x);
            st = *(const __attribute__((address_space(4))) span_words*)(tg + span_fetch_first(row8, col8, tags_x));
        } else {
            const uint32_t mine = row8 * tags_x + (tags_x ? col8 : 0u);
            const uint32_t first = wide ? mine - span_role(col8) : mine, step = wide ? 1u : 0u;
            st.x = tg[first]; st.y = tg[first + step]; st.z = tg[first + 2u * step]; st.w = tg[first + 3u * step];
            own = mine - first;                                   // (the block's own is one of the four)
            tag = own == 0u ? st.x : (own == 1u ? st.y : (own == 2u ? st.z : st.w));
        }
        tag_all = tg[P.tags_per_frame - 1u];
    }
    // ... and so does the frame's part of ray generation (camera, hoisted constants, strip assignment), in one batch
    RayGenConsts g;
    float cam_right[3];
    int shard_rank;
    uint32_t box = 0u;
    if constexpr (kVerdict) SlotOf<true>::head_no_box(P, frame, g, cam_right, shard_rank);
    else {
        SlotOf<TABLE>::head(P, frame, g, cam_right, shard_rank, box);
        asm volatile("" : "+s"(box));
    }
    // (one scalar from here on, not three: past 80 scalar registers a SIMD holds 7 of these waves, not 8)
    // (bit 0: the block has no tag; bit 1: its span may take the span path; bit 2: none of the span's blocks has a tag)
    uint32_t untagged = 0u;
    if (kVerdict) {}
    else if (kOneFetch) untagged = (uint32_t)__builtin_amdgcn_readfirstlane((int)span_verdict(st.x, st.y, st.z, st.w, own, wide, span_w, tag_all, tile_gen));
    else untagged = (uint32_t)__builtin_amdgcn_readfirstlane(((tag != tile_gen && tag_all != tile_gen) ? 1 : 0) | (span_w ? 2 : 0) |
                                                             (span_untagged(st.x, st.y, st.z, st.w, tag_all, tile_gen) ? 4 : 0));
    const uint4 boxr = make_uint4(box & 0xFFu, (box >> 8) & 0xFFu, (box >> 16) & 0xFFu, box >> 24);
    float crx = cam_right[0], cry = cam_right[1], crz = cam_right[2];
    float rcp_w = P.rcp_w, rcp_h = P.rcp_h;
    int fast_div = P.fast_screen_div;
    asm volatile("" : "+s"(g.cd.x), "+s"(g.cd.y), "+s"(g.cd.z), "+s"(g.planeV.x), "+s"(g.planeV.y), "+s"(g.planeV.z), "+s"(g.jx), "+s"(g.jy),
                      "+s"(g.W), "+s"(g.H), "+s"(crx), "+s"(cry), "+s"(crz), "+s"(shard_rank),
                      "+s"(rcp_w), "+s"(rcp_h), "+s"(fast_div));
    if (!tile_origin(M, ty, tx, shard_rank, x0, y0, yp0)) return;
    constexpr bool kLds = OCC_LDS && (TRAV == VRT_TRAVERSAL_BITMASK || TRAV == VRT_TRAVERSAL_JUMP);
    const OccT<kLds> occ = stage_occ<kLds>(P, lds_occ);

    // wave w -> 8x8 block (w&1, w>>1) of the tile (one-wave workgroups: w = 0); lane -> (l&7, l>>3).
    // (A 16x4 block would make every store of the 4-byte planes a full 64-byte line, but measured 3 % slower:
    // the wider footprint lowers the wave-wide clearance minimum by more than the stores gain.)
    // (the wave index through readfirstlane: the compiler then knows the block's origin, the rectangle test and the tag test
    // below are scalar -- a branch, not an EXEC mask around the traversal)
    int lane = threadIdx.x & 63;
    const int px0 = x0 + (wave & 1) * 8, py0 = y0 + (wave >> 1) * 8;       // the wave's 8x8 block (wave-uniform)
    // where the four blocks of the wave's 32x8 span all are skip blocks (below), the four waves trade pixels: each takes two whole
    // rows of the span (vrt_span.h; every wave of the span reaches this verdict from the same words)
    // (ONE rectangle test for both questions -- the span's blocks share the 32-pixel column and the row -- and one scalar from
    // here on: bit 0: the block is a skip block, bit 1: so is every block of its span)
    uint32_t verdict = 0u;
    if (kVerdict) verdict = (uint32_t)__builtin_amdgcn_readfirstlane((int)(vword >> verdict_shift(role)));
    if (kOneFetch) verdict = (uint32_t)__builtin_amdgcn_readfirstlane((int)span_decide(untagged, box, (uint32_t)px0, (uint32_t)py0));
    const bool span = (kVerdict || kOneFetch) ? (verdict & 2u) != 0u
                                : (untagged & 2u) != 0u && block_skips(box, (uint32_t)px0 & ~31u, (uint32_t)py0, (untagged & 4u) != 0u);
    int px, py;
    // (with a verdict the role is at hand as col8 & 3: not derived from the block's pixel column again)
    span_pixel(span, span ? (uint32_t)px0 & ~31u : (uint32_t)px0, (uint32_t)py0, kVerdict ? role : span_role((uint32_t)px0 >> 3), (uint32_t)lane, px, py);
    int W = M.W, H = M.H;
    if (px >= W || py >= H) return;
    // (two vector registers from here on, whatever they were made from: without this the megakernels' register allocation
    // changes with the choice above and the bounce chain spills one register more)
    asm volatile("" : "+v"(px), "+v"(py));
    // A skip block of a frame that has a miss-colour plane (vrt_miss_plane.h; bits 2 - 4 of the verdict byte: which of the launch's
    // planes, 0 = none): the pixel's colour word is in the plane -- no ray is generated, no texel decided.  The plane's address is
    // one of the four in front of the verdicts (k_block_verdicts put them there), requested in one batch with the planes a miss is
    // stored to.  Ahead of ray generation, which these waves have no use for.
    if constexpr (kVerdict) {
        const uint32_t which = (verdict >> 2) & 7u;
        if ((verdict & 1u) != 0u && which != 0u) {
            const_u32_ptr hp = (const_u32_ptr)((const __attribute__((address_space(4))) char*)P.verdicts - VRT_VERDICT_HEAD + 8u * (which - 1u));
            asm volatile("" : "+s"(hp));
            const MissPlanes f = SlotOf<true>::miss_planes(P, frame);
            uint32_t pw[2] = {hp[0], hp[1]};
            asm volatile("" :: "s"(f.color8), "s"(f.position), "s"(pw[0]), "s"(pw[1]));      // (one batch, one wait)
            const uint32_t* plane;
            __builtin_memcpy(&plane, pw, 8);
            const uint32_t i32 = (uint32_t)py * (uint32_t)W + (uint32_t)px;
            const uint32_t c8 = *gptr<const uint32_t>(plane, i32 << 2);
            store_miss_pixel(f, M.flags, span, i32, c8, ((uint32_t)(yp0 + (py - y0)) * (uint32_t)W + (uint32_t)px) << 2);
            return;
        }
    }
    size_t i = (size_t)py * (size_t)W + (size_t)px;

    const DevScene& s = P.sc;
    f3 start = mk3(0.0f, 0.0f, 0.0f);
    const f3 v = primary_v(g, crx, cry, crz, rcp_w, rcp_h, fast_div, px, py);
    RayHit h; RayInt r;
    // a wave whose 8x8 pixels lie outside the frame's box rectangle (FrameSlot::box, vrt_internal.h box_rect) cannot meet the
    // volume: it writes what a miss writes without testing the box (wave-uniform: the rectangle is in units of 32 pixels) --
    // and inside the rectangle neither can a wave whose block no occupied 4^3 cell of the volume projects onto (k_tile_tags)
    const bool skip = (kVerdict || kOneFetch) ? (verdict & 1u) != 0u
                                : box != 0xFF00FF00u && ((uint32_t)(px0 >> 5) < boxr.x || (uint32_t)(px0 >> 5) >= boxr.y || (uint32_t)(py0 >> 5) < boxr.z ||
                                                         (uint32_t)(py0 >> 5) >= boxr.w || (untagged & 1u) != 0u);
    // ... and of everything normalize(), atan() and asin() compute for such a pixel only the sky TEXEL is ever seen: vrt_sky.h
    // decides it from the unnormalised direction with a bound on its distance to the spec's own coordinate; a wave in which
    // some lane lies within that bound of a texel edge goes the long way round, every other wave stores the miss pixel here
    // (32-bit byte offsets from the plane pointers: one shift per plane instead of a 64-bit address each)
    f3 dir;
    if (skip) {
    if (M.flags & VRT_MAPFLAG_SKY_FAST) {
        // (everything the short path reads -- the texel constants, the RGBA8 sky, the eight planes a miss is stored to -- is
        // requested HERE in one batch, through pointers the compiler cannot see through: hoisted to the top of the kernel with
        // the other arguments they would be 28 more scalar registers live across ray generation, one wave per SIMD less for
        // every wave of the kernel; read one after the other where each is used they are three dependent round trips in a
        // wave that does little else)
        SkyFastConsts k;
        const uint32_t* sky8;
        {
            const_u32_ptr kp = kernarg_words(offsetof(GeomParams, sc) + offsetof(DevScene, sky8));
            static_assert(offsetof(DevScene, skyk) == offsetof(DevScene, sky8) + 8 && sizeof(SkyFastConsts) == 40, "sky8 and skyk are read as one block");
            uint32_t tmp[12];
#pragma unroll
            for (int q = 0; q < 12; q++) tmp[q] = kp[q];
            __builtin_memcpy(&sky8, tmp, 8);
            __builtin_memcpy(&k, tmp + 2, sizeof k);
        }
        const MissPlanes f = SlotOf<TABLE>::miss_planes(P, frame);
        uint32_t tx, ty;
        const bool sure = sky_texel_fast(v.x, v.y, v.z, k, tx, ty);
        if (__ballot(!sure) == 0ull) {
            // (the pointers were assembled from words, so the compiler no longer knows they are global memory: say so, or every
            // access below is a flat instruction with a 64-bit address in two vector registers)
            const uint32_t c8 = *gptr<const uint32_t>(sky8, (ty * k.w + tx) << 2);
            const uint32_t i32 = (uint32_t)py * (uint32_t)W + (uint32_t)px;
            // (span path: the planes of zeros as NON-TEMPORAL stores -- a whole 128-byte row per instruction has nothing left to merge
            // in the L2, which the 32-byte pieces of an 8x8 block do: those measured 4.88 against 3.2 ms this way)
            // (the primary-only kernels, where it was measured; in the megakernels a scalar that lives this long costs the bounce
            // chain a spilled register more)
            if (MODE == 1 && span && (M.flags & VRT_MAPFLAG_SIX)) {
                __builtin_nontemporal_store((vrt_f4){0.0f, 0.0f, 0.0f, 0.0f}, gptr<vrt_f4>(f.position, i32 << 4));
                __builtin_nontemporal_store((vrt_f2){0.0f, 0.0f}, gptr<vrt_f2>(f.motion, i32 << 3));
                __builtin_nontemporal_store(0.0f, gptr<float>(f.depth, i32 << 2));
                __builtin_nontemporal_store(0u, gptr<uint32_t>(f.normal8, i32 << 2));
                __builtin_nontemporal_store((uint8_t)0, gptr<uint8_t>(f.mask8, i32));
                *gptr<uint32_t>(f.color8, i32 << 2) = c8;
                return;
            }
            if (M.flags & VRT_MAPFLAG_SIX) {                       // the reference's six targets and nothing else: six stores, no pointer tested
                *gptr<vrt_f4>(f.position, i32 << 4) = (vrt_f4){0.0f, 0.0f, 0.0f, 0.0f};
                *gptr<vrt_f2>(f.motion, i32 << 3) = (vrt_f2){0.0f, 0.0f};
                *gptr<float>(f.depth, i32 << 2) = 0.0f;
                *gptr<uint32_t>(f.normal8, i32 << 2) = 0u;
                *gptr<uint8_t>(f.mask8, i32) = (uint8_t)0;
                *gptr<uint32_t>(f.color8, i32 << 2) = c8;
                return;
            }
            if (f.position) *gptr<vrt_f4>(f.position, i32 << 4) = (vrt_f4){0.0f, 0.0f, 0.0f, 0.0f};
            if (f.motion) *gptr<vrt_f2>(f.motion, i32 << 3) = (vrt_f2){0.0f, 0.0f};
            if (f.depth) *gptr<float>(f.depth, i32 << 2) = 0.0f;
            if (f.normal8) *gptr<uint32_t>(f.normal8, i32 << 2) = 0u;
            if (f.mask8) *gptr<uint8_t>(f.mask8, i32) = (uint8_t)0;
            if (f.hit_id) *gptr<uint8_t>(f.hit_id, i32) = (uint8_t)0;
            if (f.color8) *gptr<uint32_t>(f.color8, i32 << 2) = c8;
            if (f.color8_strips) *gptr<uint32_t>(f.color8_strips, ((uint32_t)(yp0 + (py - y0)) * (uint32_t)W + (uint32_t)px) << 2) = c8;
            return;
        }
    }
        dir = primary_normalize(v);
        h.material = 0u; h.dir = dir; h.pos = mk3(0.0f, 0.0f, 0.0f); h.normal = mk3(0.0f, 0.0f, 0.0f); h.ncode = 0xFFFFFFFFu;
        r.material = 0u; r.mask = 0u; r.fetches = 0u; r.mx = r.my = r.mz = 0; r.dbg0 = 1u; r.dbg1 = 0u;
    } else {
        // (the scene scalars the DDA set-up will ask for one by one: requested here, used from these registers later)
        asm volatile("" :: "s"(P.sc.vol.W), "s"(P.sc.vol.H), "s"(P.sc.vol.D), "s"(P.st.max_steps), "s"(P.sc.vol.df), "s"(P.sc.vol.df_stride),
                           "s"(P.sc.vol.vox));
        start = SlotOf<TABLE>::cam_pos(P, frame);
        dir = primary_normalize(v);
        trace_ray<TRAV, OccT<kLds>, MODE == 1, false, MODE == 1>(s, occ, start, dir, P.st.max_steps, h, r);   // look-ahead request: primary-only kernel
    }
    bool hit = h.material != 0;

    const vrt_frame f = SlotOf<TABLE>::planes(P, frame);   // by value: the fourteen plane pointers arrive with two scalar loads, not one by one before each store
    float depth = 0.0f;
    if (hit) depth = len3(mk3(h.pos.x - start.x, h.pos.y - start.y, h.pos.z - start.z));
    // (the reference's targets through 32-bit byte offsets from pointers SAID to be global memory -- the table form assembles
    // them from words and would otherwise get flat instructions with a 64-bit address each; the host admits frames below
    // 2^28 pixels)
    const uint32_t i32 = (uint32_t)i;
    // (the launch's flags once more from the kernel's own arguments: a scalar register held across the march would be the 77th)
    const bool six = (kernarg_words(offsetof(GeomParams, map) + offsetof(TileMap, flags))[0] & VRT_MAPFLAG_SIX) != 0u;
    if (six) {                                                  // the reference's six targets and nothing else (the colour below)
        uint32_t n = 0u;
        if (hit) n = (uint32_t)(uint8_t)snorm8(h.normal.x) | ((uint32_t)(uint8_t)snorm8(h.normal.y) << 8) | ((uint32_t)(uint8_t)snorm8(h.normal.z) << 16);
        *gptr<float>(f.depth, i32 << 2) = depth;
        *gptr<vrt_f2>(f.motion, i32 << 3) = (vrt_f2){0.0f, 0.0f};
        *gptr<uint8_t>(f.mask8, i32) = hit ? (uint8_t)230 : (uint8_t)0;
        *gptr<vrt_f4>(f.position, i32 << 4) = (vrt_f4){h.pos.x, h.pos.y, h.pos.z, 0.0f};
        *gptr<uint32_t>(f.normal8, i32 << 2) = n;
    } else {
    if (f.depth) *gptr<float>(f.depth, i32 << 2) = depth;
    if (f.motion) *gptr<vrt_f2>(f.motion, i32 << 3) = (vrt_f2){0.0f, 0.0f};
    if (f.mask8) *gptr<uint8_t>(f.mask8, i32) = hit ? (uint8_t)230 : (uint8_t)0;          // unorm8(0.9f) = 230 (tests/test_oracle_kat.py), unorm8(0) = 0
    if (f.position) *gptr<vrt_f4>(f.position, i32 << 4) = (vrt_f4){h.pos.x, h.pos.y, h.pos.z, 0.0f};
    if (f.normal8) {
        uint32_t n = 0u;                                                    // miss: normal = 0; a wave without a hit skips the conversions
        if (hit) n = (uint32_t)(uint8_t)snorm8(h.normal.x) | ((uint32_t)(uint8_t)snorm8(h.normal.y) << 8) | ((uint32_t)(uint8_t)snorm8(h.normal.z) << 16);
        *gptr<uint32_t>(f.normal8, i32 << 2) = n;
    }
    if (f.hit_id) *gptr<uint8_t>(f.hit_id, i32) = (uint8_t)h.material;
    if (f.hit_voxel) {
        f.hit_voxel[i * 3 + 0] = hit ? (int16_t)r.mx : (int16_t)0;
        f.hit_voxel[i * 3 + 1] = hit ? (int16_t)r.my : (int16_t)0;
        f.hit_voxel[i * 3 + 2] = hit ? (int16_t)r.mz : (int16_t)0;
    }
    if (f.hit_mask) f.hit_mask[i] = hit ? (uint8_t)r.mask : (uint8_t)0;
    if (VRT_COUNTS(TRAV) && f.steps_primary) f.steps_primary[i] = r.fetches;
    if (VRT_COUNTS(TRAV) && f.steps_total) f.steps_total[i] = (P.st.flags & VRT_FLAG_DEBUG_PLANES) ? r.dbg0 : r.fetches;
    if (f.rays_total) f.rays_total[i] = (P.st.flags & VRT_FLAG_DEBUG_PLANES) ? r.dbg1 : 1u;
    if ((P.st.flags & 2u) && f.steps_total && f.rays_total) {             // wave start / end stamps, 10 ns units
        f.steps_total[i] = (uint32_t)t_begin;
        f.rays_total[i] = (uint32_t)wall_clock64();
    }
    }
    uint32_t* const steps_total = six ? nullptr : f.steps_total; uint32_t* const rays_total = six ? nullptr : f.rays_total;

    // primary rays only: a hit's colour is an entry of the launch's table (GeomParams::hit_colors: colorHit() of every material
    // and normal, made by colorHit() itself); a wave one of whose hits has none of the 26 normals computes as before
    if (MODE == 1) {
        const uint32_t* const hc = P.hit_colors;
        if (hc && !f.color_f && __ballot(hit && h.ncode == 0xFFFFFFFFu) == 0ull) {
            uint32_t c8;
            if (hit) c8 = *gptr<const uint32_t>(hc, ((h.material << 6) | h.ncode) << 2);
            else {
                const f3 col = sky_color(s, dir);
                c8 = (uint32_t)unorm8(col.x) | ((uint32_t)unorm8(col.y) << 8) | ((uint32_t)unorm8(col.z) << 16);
            }
            if (six) { *gptr<uint32_t>(f.color8, i32 << 2) = c8; return; }
            if (f.color8) *gptr<uint32_t>(f.color8, i32 << 2) = c8;
            if (f.color8_strips) *gptr<uint32_t>(f.color8_strips, ((uint32_t)(yp0 + (py - y0)) * (uint32_t)W + (uint32_t)px) << 2) = c8;
            return;
        }
    }
    if (MODE != 0) {                                           // 1: primary only; 2: megakernel; 4: megakernel, nothing can bounce
        f3 col;
        if (MODE >= 5) {
            // The packed chain is wave-uniform: in a wave with a hit EVERY lane goes through it, the lanes that missed (and those whose chain
            // has ended) for the AO rays' sake -- they draw on the wave's pool like the others (secondary_rays); what they return is not
            // used.  (The other forms keep the divergent call: with helpers at the primary hit alone the megakernel without its bounce
            // loop needs 67 VGPRs instead of 64 and the reference defaults measured 132.8 against 128 us, config 5 3.32 against 3.07 ms.)
            PixCtx c; c.px = px; c.py = py; c.fetches = 0; c.rays = 0; c.pc = SlotOf<TABLE>::push(P, frame);
            c.ldsw = (uint32_t)(uintptr_t)(lds_u64_ptr)lds_occ + (uint32_t)wave * (uint32_t)VRT_AO_SLOT;   // (the hand-written loop's kernels are launched with a pool per wave)
            f3 colh = mk3(0.0f, 0.0f, 0.0f);
            if (__ballot(hit) != 0ull) colh = color_main_ray_packed<TRAV, OccT<kLds>, (MODE == 5 ? 2 : (MODE == 6 ? 5 : VRT_MAX_BOUNCES))>(P, occ, c, h, hit);
            if (hit) {
                col = colh;
                if (VRT_COUNTS(TRAV) && steps_total && !(P.st.flags & 3u)) steps_total[i] = r.fetches + c.fetches;
                if (rays_total && !(P.st.flags & 3u)) rays_total[i] = 1u + c.rays;
            } else {
                col = sky_color(s, dir);
                // (VRT_FLAG_LOOKUP_COUNTS: the bytes a lane asked for while it helped with the others' AO rays belong to the frame's sum)
                if (VRT_COUNTS(TRAV) && steps_total && P.sc.vol.count_lookups != 0u && !(P.st.flags & 3u)) steps_total[i] = r.fetches + c.fetches;
            }
        } else if (hit) {
            PixCtx c; c.px = px; c.py = py; c.fetches = 0; c.rays = 0; c.pc = SlotOf<TABLE>::push(P, frame);
            c.ldsw = (uint32_t)(uintptr_t)(lds_u64_ptr)lds_occ + (uint32_t)wave * (uint32_t)VRT_AO_SLOT;
            if (MODE == 1) col = color_hit<TRAV, OccT<kLds>, false>(P, occ, c, h, mk3(0.0f, 0.0f, 0.0f), 0);   // ambient = 1, unshadowed, no reflection
            else {
                col = color_main_ray<TRAV, OccT<kLds>, MODE != 4>(P, occ, c, h);
                if (VRT_COUNTS(TRAV) && steps_total && !(P.st.flags & 3u)) steps_total[i] = r.fetches + c.fetches;
                if (rays_total && !(P.st.flags & 3u)) rays_total[i] = 1u + c.rays;
            }
        } else {
            col = sky_color(s, dir);
        }
        store_color(f, col, i, i32, ((uint32_t)(yp0 + (py - y0)) * (uint32_t)W + (uint32_t)px) << 2);
    } else if (hit) {
        // hit record for K2 (position bits + material | mask << 8 | (step+1) codes) and a slot in the compacted list of
        // hit pixels: K2 then runs one lane per HIT pixel instead of one per pixel (hipcc folds the per-lane
        // atomicAdd into one atomic per wave)
        uint32_t packed = h.material | (r.mask << 8) | ((uint32_t)(r.sx + 1) << 11) | ((uint32_t)(r.sy + 1) << 13) |
                          ((uint32_t)(r.sz + 1) << 15);
        P.records[i] = make_uint4(__float_as_uint(h.pos.x), __float_as_uint(h.pos.y), __float_as_uint(h.pos.z), packed);
        uint32_t slot = atomicAdd(P.hit_count, 1u);
        P.hit_list[slot] = (uint32_t)i;
    } else {
        // misses are final here: colorMainRay is never reached (voxel_volume.frag:337-345)
        store_color(f, sky_color(s, dir), i, i32, ((uint32_t)(yp0 + (py - y0)) * (uint32_t)W + (uint32_t)px) << 2);
    }
}

// ---------------------------------------------------------------------------------------------
// K2: secondary rays + shading
// ---------------------------------------------------------------------------------------------

template <int TRAV, bool OCC_LDS>
__global__ __launch_bounds__(256) void k_shade(const GeomParams P)
{
    extern __shared__ __attribute__((aligned(16))) uint64_t lds_occ[];
    constexpr bool kLds = OCC_LDS && (TRAV == VRT_TRAVERSAL_BITMASK || TRAV == VRT_TRAVERSAL_JUMP);
    uint32_t count = *P.hit_count;                        // written by K1 (previous kernel on the stream)
    if (blockIdx.x * 256u >= count) return;               // uniform per workgroup
    const OccT<kLds> occ = stage_occ<kLds>(P, lds_occ);
    uint32_t gid = blockIdx.x * 256u + threadIdx.x;
    if (gid >= count) return;
    size_t i = P.hit_list[gid];
    int W = P.W;
    int px = (int)(i % (size_t)W), py = (int)(i / (size_t)W);

    uint4 rec = P.records[i];
    RayHit h;
    h.material = rec.w & 0xFFu;
    h.dir = primary_dir(P.slot[0], px, py);
    h.pos = mk3(__uint_as_float(rec.x), __uint_as_float(rec.y), __uint_as_float(rec.z));
    uint32_t mask = (rec.w >> 8) & 7u;
    int sx = (int)((rec.w >> 11) & 3u) - 1, sy = (int)((rec.w >> 13) & 3u) - 1, sz = (int)((rec.w >> 15) & 3u) - 1;
    PixCtx c; c.px = px; c.py = py; c.fetches = 0; c.rays = 0; c.pc = &P.slot[0].pc;
    c.ldsw = (uint32_t)(uintptr_t)(lds_u64_ptr)lds_occ + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) * (uint32_t)VRT_AO_SLOT;
    h.normal = hit_normal(mask, sx, sy, sz);
    {
        const bool general = (mask & 7u) == 0u || ((mask & 1u) && sx == 0) || ((mask & 2u) && sy == 0) || ((mask & 4u) && sz == 0);
        h.ncode = general ? 0xFFFFFFFFu : ((mask & 7u) | ((uint32_t)(sx < 0) << 3) | ((uint32_t)(sy < 0) << 4) | ((uint32_t)(sz < 0) << 5));
    }
    f3 col = color_main_ray<TRAV>(P, occ, c, h);
    const vrt_frame& f = P.slot[0].fr;
    if (f.color_f) { f.color_f[i * 3 + 0] = col.x; f.color_f[i * 3 + 1] = col.y; f.color_f[i * 3 + 2] = col.z; }
    if (f.color8 || f.color8_strips) {
        uchar4 c8; c8.x = unorm8(col.x); c8.y = unorm8(col.y); c8.z = unorm8(col.z); c8.w = 0;
        if (f.color8) reinterpret_cast<uchar4*>(f.color8)[i] = c8;
        if (f.color8_strips) {                 // the split form has no tile: row -> packed row by division
            int strip = py / P.sh.strip_rows;
            int yp = (strip / P.sh.nranks) * P.sh.strip_rows + (py - strip * P.sh.strip_rows);
            reinterpret_cast<uchar4*>(f.color8_strips)[(size_t)yp * (size_t)P.W + (size_t)px] = c8;
        }
    }
    if (VRT_COUNTS(TRAV) && f.steps_total) f.steps_total[i] += c.fetches;
    if (f.rays_total) f.rays_total[i] += c.rays;
}

// ---------------------------------------------------------------------------------------------
// launch plumbing for K1 / K2
// ---------------------------------------------------------------------------------------------

// K1 of one MODE and TABLE, with the tile map's form as a compile-time constant for the product traversals (block_to_tile; their
// counting twins: the general tile map only -- fewer kernels to build)
template <int TRAV, bool OCC_LDS, int MODE, bool TABLE>
static void launch_k1_map(const GeomParams& p, dim3 grid, dim3 block, size_t lds, hipStream_t s)
{
    if constexpr (TRAV == VRT_TRAVERSAL_DF_FAST || TRAV == VRT_TRAVERSAL_BRICK) {
        if (p.xcd_turn == 0) { hipLaunchKernelGGL((k_primary<TRAV, OCC_LDS, MODE, TABLE, 0>), grid, block, lds, s, p); return; }
        if (p.xcd_turn == 2) { hipLaunchKernelGGL((k_primary<TRAV, OCC_LDS, MODE, TABLE, 2>), grid, block, lds, s, p); return; }
    }
    hipLaunchKernelGGL((k_primary<TRAV, OCC_LDS, MODE, TABLE, -1>), grid, block, lds, s, p);
}

// K1 with the slots in the table or in the kernel arguments: its MODE.  MODE 0 (the split form) exists only without a table: it
// renders one frame per launch.
template <int TRAV, bool OCC_LDS, bool TABLE>
static hipError_t launch_k1(const GeomParams& p, dim3 grid, dim3 block, size_t lds, hipStream_t s)
{
    constexpr bool kProduct = TRAV == VRT_TRAVERSAL_DF_FAST || TRAV == VRT_TRAVERSAL_DF_FAST_CNT || TRAV == VRT_TRAVERSAL_BRICK || TRAV == VRT_TRAVERSAL_BRICK_CNT;
    if (p.fused_shade == 1) {
        if (TABLE && !p.verdicts) return hipErrorInvalidValue;    // the primary-only kernels of table launches read their blocks' verdicts (k_block_verdicts)
        launch_k1_map<TRAV, OCC_LDS, 1, TABLE>(p, grid, block, lds, s);
    }
    else if (p.fused_shade == 2) {
        if (p.no_bounce) launch_k1_map<TRAV, OCC_LDS, 4, TABLE>(p, grid, block, lds, s);
        else if (kProduct && p.packed_chain) {
            if constexpr (kProduct) {
                if (p.st.max_bounces <= 2)      launch_k1_map<TRAV, OCC_LDS, 5, TABLE>(p, grid, block, lds, s);
                else if (p.st.max_bounces <= 5) launch_k1_map<TRAV, OCC_LDS, 6, TABLE>(p, grid, block, lds, s);
                else                            launch_k1_map<TRAV, OCC_LDS, 7, TABLE>(p, grid, block, lds, s);
            }
        }
        else launch_k1_map<TRAV, OCC_LDS, 2, TABLE>(p, grid, block, lds, s);
    }
    else if constexpr (TABLE) return hipErrorInvalidValue;      // the split form renders one frame per launch and never gets here
    else launch_k1_map<TRAV, OCC_LDS, 0, false>(p, grid, block, lds, s);
    return hipGetLastError();
}

template <int TRAV, bool OCC_LDS>
hipError_t launch_primary_t(const GeomParams& p, hipStream_t s)
{
    // (block_to_tile: three-dimensional grids whose x extent is a multiple of 8 for xcd_turn 0 and 2, a line for xcd_turn 1)
    dim3 grid((unsigned)p.tiles_x * 8u, (unsigned)((p.tiles_y_local + 7) / 8), (unsigned)p.n_frames);
    if (p.xcd_turn == 2) grid = dim3(8u * (((unsigned)p.tiles_x + 1u) / 2u), ((unsigned)p.tiles_y_local + 3u) / 4u, (unsigned)p.n_frames);
    else if (p.xcd_turn) grid = dim3((unsigned)p.tiles_x * 8u * (unsigned)((p.tiles_y_local * p.n_frames + 7) / 8));
    dim3 block(p.tile_h == 8 ? 64 : 256);
    size_t lds = (OCC_LDS && (TRAV == VRT_TRAVERSAL_BITMASK || TRAV == VRT_TRAVERSAL_JUMP)) ? p.occ2_bytes + p.occ3_bytes : 0;
    // (the hand-written loop's AO batches: VRT_AO_SLOT bytes per wave, the contract at the head of vrt_shade.h)
    if ((TRAV == VRT_TRAVERSAL_DF_FAST || TRAV == VRT_TRAVERSAL_DF_FAST_CNT || TRAV == VRT_TRAVERSAL_BRICK || TRAV == VRT_TRAVERSAL_BRICK_CNT) && p.fused_shade != 1)
        lds = (size_t)(block.x / 64u) * (size_t)VRT_AO_SLOT;
    return p.table ? launch_k1<TRAV, OCC_LDS, true>(p, grid, block, lds, s) : launch_k1<TRAV, OCC_LDS, false>(p, grid, block, lds, s);
}

template <int TRAV, bool OCC_LDS>
hipError_t launch_shade_t(const GeomParams& p, hipStream_t s)
{
    // one lane per hit pixel of the compacted list; sized for the worst case (every local pixel hit), surplus
    // workgroups leave at once
    dim3 grid((unsigned)(((size_t)p.total_tiles * p.tile_w * p.tile_h + 255) / 256)), block(256);
    size_t lds = (OCC_LDS && (TRAV == VRT_TRAVERSAL_BITMASK || TRAV == VRT_TRAVERSAL_JUMP)) ? p.occ2_bytes + p.occ3_bytes : 0;
    if (TRAV == VRT_TRAVERSAL_DF_FAST || TRAV == VRT_TRAVERSAL_DF_FAST_CNT || TRAV == VRT_TRAVERSAL_BRICK || TRAV == VRT_TRAVERSAL_BRICK_CNT) lds = 4u * (size_t)VRT_AO_SLOT;
    hipLaunchKernelGGL((k_shade<TRAV, OCC_LDS>), grid, block, lds, s, p);
    return hipGetLastError();
}

// This file is compiled once per part, -DVRT_K1_PART=n -> vrt_device_n.o (Makefile): the K1 and K2 kernels of the eleven
// (traversal, occ_in_lds) pairs are spread over the parts below, and part 0 also holds everything that is not a template.
// Every part sees all eleven launchers as `extern template` and defines its own.
#define VRT_K1_K2(EXT, TRAV, OCC_LDS)                                                          \
    EXT template hipError_t launch_primary_t<TRAV, OCC_LDS>(const GeomParams&, hipStream_t);   \
    EXT template hipError_t launch_shade_t<TRAV, OCC_LDS>(const GeomParams&, hipStream_t);
#define VRT_PART_0(EXT) VRT_K1_K2(EXT, VRT_TRAVERSAL_BRICK, false)
#define VRT_PART_1(EXT) VRT_K1_K2(EXT, VRT_TRAVERSAL_DF_FAST, false)
#define VRT_PART_2(EXT) VRT_K1_K2(EXT, VRT_TRAVERSAL_DF_FAST_CNT, false) VRT_K1_K2(EXT, VRT_TRAVERSAL_BRICK_CNT, false)
#define VRT_PART_3(EXT) VRT_K1_K2(EXT, VRT_TRAVERSAL_DENSE, false) VRT_K1_K2(EXT, VRT_TRAVERSAL_DF, false) VRT_K1_K2(EXT, VRT_TRAVERSAL_DFJ, false) \
                        VRT_K1_K2(EXT, VRT_TRAVERSAL_BITMASK, false) VRT_K1_K2(EXT, VRT_TRAVERSAL_BITMASK, true)                                     \
                        VRT_K1_K2(EXT, VRT_TRAVERSAL_JUMP, false) VRT_K1_K2(EXT, VRT_TRAVERSAL_JUMP, true)
VRT_PART_0(extern) VRT_PART_1(extern) VRT_PART_2(extern) VRT_PART_3(extern)
#define VRT_PART_N(N) VRT_PART_##N
#define VRT_PART(N) VRT_PART_N(N)
VRT_PART(VRT_K1_PART)()

#if VRT_K1_PART == 0      // everything below: in one object only

// skyColor of every normal a hit can have, by sky_color itself (so that the table holds bit for bit what the shading code
// would compute); entry = mask | (sx<0)<<3 | (sy<0)<<4 | (sz<0)<<5, 64 x float4
__global__ void k_sky_normals(const DevScene s, float4* table)
{
    const uint32_t code = threadIdx.x & 63u, mask = code & 7u;
    const int sx = (code & 8u) ? -1 : 1, sy = (code & 16u) ? -1 : 1, sz = (code & 32u) ? -1 : 1;
    f3 c = mk3(0.0f, 0.0f, 0.0f);
    if (mask != 0u) c = sky_color(s, hit_normal(mask, sx, sy, sz));
    table[code] = make_float4(c.x, c.y, c.z, 0.0f);
}

hipError_t launch_sky_normals(const DevScene& sc, float* table, hipStream_t s)
{
    hipLaunchKernelGGL(k_sky_normals, dim3(1), dim3(64), 0, s, sc, reinterpret_cast<float4*>(table));
    return hipGetLastError();
}

// the sky as the colour target stores it: unorm8 of r, g, b per texel (a = 0, canonical rule F)
__global__ __launch_bounds__(256) void k_sky_rgba8(const float4* __restrict__ sky, uint32_t* __restrict__ sky8, size_t n)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 t = sky[i];
    sky8[i] = (uint32_t)unorm8(t.x) | ((uint32_t)unorm8(t.y) << 8) | ((uint32_t)unorm8(t.z) << 16);
}

hipError_t launch_sky_rgba8(const float* sky, uint32_t* sky8, size_t n, hipStream_t s)
{
    hipLaunchKernelGGL(k_sky_rgba8, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, reinterpret_cast<const float4*>(sky), sky8, n);
    return hipGetLastError();
}

// Diagnostic (vrt_debug_sky_texels): for n unnormalised directions the sky texel by the numeric spec (sky_color's own
// arithmetic) and by the fast path, as the hardware computes both: out[4i] = spec x | y << 16, [4i+1] = fast x | y << 16,
// [4i+2] = the fast path is sure, [4i+3] = float bits of the fast u * sky_w
__global__ __launch_bounds__(256) void k_debug_sky(const DevScene s, const float* __restrict__ v, size_t n, uint32_t* __restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float vx = v[3 * i], vy = v[3 * i + 1], vz = v[3 * i + 2];
    const f3 d = normalize3(mk3(vx, vy, vz));
    const float u = atan2_spec(d.z, d.x) * 0.1591f + 0.5f;
    const float w = asin_spec(-d.y) * 0.3183f + 0.5f;
    const uint32_t sx = wrap_texel(u, s.sky_w), sy = wrap_texel(w, s.sky_h);
    uint32_t tx = 0u, ty = 0u;
    float un = 0.0f, vn = 0.0f;
    const bool sure = s.skyk.w != 0u && sky_texel_fast(vx, vy, vz, s.skyk, tx, ty, un, vn);
    out[4 * i] = sx | (sy << 16); out[4 * i + 1] = tx | (ty << 16); out[4 * i + 2] = sure ? 1u : 0u; out[4 * i + 3] = __float_as_uint(un);
}

// Diagnostic (vrt_debug_spec): one primitive of vrt_spec.h per element, bit patterns in, bit patterns out -- lane i of the launch
// evaluates element i (no reordering: which elements share a wave is part of what tests/test_gpu_spec.py varies).  fn as in
// include/vrt.h; out holds one word per element, three (x, y, z) for normalize3.  Nothing is restated here: the calls below are
// the header's functions under this object's flags.
__global__ __launch_bounds__(256) void k_debug_spec(uint32_t fn, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                    const uint32_t* __restrict__ c, size_t n, uint32_t* __restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float x = __uint_as_float(a[i]);
    switch (fn) {
    case 0: out[i] = __float_as_uint(sqrt_spec(x)); break;
    case 1: out[i] = __float_as_uint(div_spec(x, __uint_as_float(b[i]))); break;
    case 2: out[i] = __float_as_uint(atan2_spec(x, __uint_as_float(b[i]))); break;
    case 3: out[i] = __float_as_uint(asin_spec(x)); break;
    case 4: out[i] = __float_as_uint(exp_spec(x)); break;
    case 5: out[i] = (uint32_t)unorm8(x); break;
    case 6: out[i] = (uint32_t)(int32_t)snorm8(x); break;
    case 7: out[i] = wrap_texel(x, b[i]); break;
    case 8: {
        const f3 d = normalize3(mk3(x, __uint_as_float(b[i]), __uint_as_float(c[i])));
        out[3 * i] = __float_as_uint(d.x); out[3 * i + 1] = __float_as_uint(d.y); out[3 * i + 2] = __float_as_uint(d.z);
        break;
    }
    default: break;
    }
}

hipError_t launch_debug_spec(uint32_t fn, const uint32_t* a, const uint32_t* b, const uint32_t* c, size_t n, uint32_t* out, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_debug_spec, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, fn, a, b, c, n, out);
    return hipGetLastError();
}

// development build (-DVRT_TRACE_COUNTERS): the brick march's look-up counters, read and reset
hipError_t debug_brick_counts(unsigned long long out[4])
{
#if defined(VRT_TRACE_COUNTERS)
    hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(g_vrt_brick_counts), 32);
    if (e != hipSuccess) return e;
    const unsigned long long zero[4] = {0, 0, 0, 0};
    return hipMemcpyToSymbol(HIP_SYMBOL(g_vrt_brick_counts), zero, 32);
#else
    out[0] = out[1] = out[2] = out[3] = 0ull;
    return hipSuccess;
#endif
}

hipError_t launch_debug_sky(const DevScene& sc, const float* v, size_t n, uint32_t* out, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_debug_sky, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, sc, v, n, out);
    return hipGetLastError();
}

// colorHit() of every (material, normal) a primary ray can hit, for launches without secondary rays (GeomParams::hit_colors)
__global__ __launch_bounds__(256) void k_hit_colors(const GeomParams P, uint32_t* table)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const uint32_t code = t & 63u, material = t >> 6, mask = code & 7u;
    const int sx = (code & 8u) ? -1 : 1, sy = (code & 16u) ? -1 : 1, sz = (code & 32u) ? -1 : 1;
    uint32_t c8 = 0u;
    if (mask != 0u && material != 0u && material < 256u) {
        RayHit h;
        h.material = material; h.pos = mk3(0.0f, 0.0f, 0.0f); h.dir = mk3(0.0f, 0.0f, 0.0f);
        h.normal = hit_normal(mask, sx, sy, sz); h.ncode = code;
        PixCtx c; c.px = 0; c.py = 0; c.fetches = 0; c.rays = 0; c.pc = nullptr; c.ldsw = 0u;
        OccT<false> occ; occ.o2 = nullptr; occ.o3 = nullptr;
        const f3 col = color_hit<VRT_TRAVERSAL_DF_FAST, OccT<false>, false>(P, occ, c, h, mk3(0.0f, 0.0f, 0.0f), 0);
        c8 = (uint32_t)unorm8(col.x) | ((uint32_t)unorm8(col.y) << 8) | ((uint32_t)unorm8(col.z) << 16);
    }
    if (t < 256u * 64u) table[t] = c8;
}

hipError_t launch_hit_colors(const GeomParams& p, uint32_t* table, hipStream_t s)
{
    hipLaunchKernelGGL(k_hit_colors, dim3(64), dim3(256), 0, s, p, table);
    return hipGetLastError();
}

// The miss-colour plane of a view (vrt_miss_plane.h): the word K1 stores in the colour target of a pixel that misses, for every pixel
// of a W x H frame, by K1's own long miss path -- primary_v, primary_normalize, sky_color, unorm8: the same functions, so the plane
// holds bit for bit what a sky wave of K1 would store (the short path's texel is the long path's wherever it is sure: vrt_sky.h).
// One lane per pixel, a workgroup per 256 pixels of a row; plain stores: the plane is read by every frame of its group.
__global__ __launch_bounds__(256) void k_miss_plane(const MissPlaneParams P)
{
    const int px = (int)(blockIdx.x * 256u + threadIdx.x), py = (int)blockIdx.y;
    if (px >= P.W) return;
    const f3 v = primary_v(P.rg, P.cam_right[0], P.cam_right[1], P.cam_right[2], P.rcp_w, P.rcp_h, P.fast_screen_div, px, py);
    const f3 col = sky_color(P.sc, primary_normalize(v));
    P.plane[(size_t)py * (size_t)P.W + (size_t)px] = (uint32_t)unorm8(col.x) | ((uint32_t)unorm8(col.y) << 8) | ((uint32_t)unorm8(col.z) << 16);
}

hipError_t launch_miss_plane(const MissPlaneParams& p, hipStream_t s)
{
    if (p.W <= 0 || p.H <= 0 || !p.plane) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_miss_plane, dim3((unsigned)((p.W + 255) / 256), (unsigned)p.H), dim3(256), 0, s, p);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Tile tags: which 8x8-pixel blocks of a frame can a primary ray meet anything in?  One lane per occupied 4^3-voxel cell of
// the volume (the scene's list of them); the cell, grown by one voxel on every side, is projected through the frame's
// camera and the blocks its screen rectangle (+ 2 pixels) touches are tagged with the launch's generation number -- plain
// stores of one value, no clearing between launches.  A block without the tag holds no pixel whose ray passes within a
// voxel of anything solid: its wave writes what a miss writes (k_primary).  Frames without a box rectangle (camera in or
// near the volume, a degenerate basis) have no tags, nor have frames with a cell closer than the projection can bound.
// ---------------------------------------------------------------------------------------------
template <bool TABLE>
__global__ __launch_bounds__(256) void k_tile_tags(const GeomParams P)
{
    const uint32_t frame = blockIdx.y;
    RayGenConsts g;
    float cam[3], U[3];
    int shard_rank;
    uint32_t box;
    SlotOf<TABLE>::head(P, frame, g, U, shard_rank, box);
    if (box == 0xFF00FF00u) return;
    { const f3 cp = SlotOf<TABLE>::cam_pos(P, frame); cam[0] = cp.x; cam[1] = cp.y; cam[2] = cp.z; }
    const uint32_t ci = blockIdx.x * 256u + threadIdx.x;
    if (ci >= P.n_cells) return;
    const uint32_t cell = P.cells[ci];
    const uint32_t cs = P.cell_size;                            // 4 (dense scenes: the cells of the 16^3 summaries' bits) or 8 (bricks)
    const float ext = (float)cs + 2.0f;
    const float lo[3] = {(float)((cell & 1023u) * cs) - 1.0f, (float)(((cell >> 10) & 1023u) * cs) - 1.0f, (float)((cell >> 20) * cs) - 1.0f};
    uint32_t* tags = P.tile_tags + (size_t)frame * P.tags_per_frame;
    // the cell's screen rectangle and the bound on its error (vrt_tags.h: the projection, its rounding analysis and the rule
    // that a rectangle is only used while its bound is below what the two pixels of margin absorb)
    TagCam tc;
    tc.U[0] = U[0]; tc.U[1] = U[1]; tc.U[2] = U[2];
    tc.V[0] = g.planeV.x; tc.V[1] = g.planeV.y; tc.V[2] = g.planeV.z;
    tc.C[0] = g.cd.x + g.jx; tc.C[1] = g.cd.y + g.jy; tc.C[2] = g.cd.z;
    tc.cam[0] = cam[0]; tc.cam[1] = cam[1]; tc.cam[2] = cam[2];
    tc.W = g.W; tc.H = g.H;
    // a rank that owns ONE band of rows (the banded assignment of a multi-GPU batch): seven cells in eight of an 8-GPU step lie
    // outside it, and two linear forms say so without the eight corners' divisions (vrt_tags.h tag_band_cull, with its own bound)
    if (P.sh.nranks > 1) {
        const int rows = P.sh.strip_rows, total = ((int)g.H + rows - 1) / rows;
        if (shard_rank + P.sh.nranks >= total && tag_band_cull(tc, lo, ext, (float)(shard_rank * rows), (float)(shard_rank * rows + rows))) return;
    }
    float x0, x1, y0, y1, ex, ey;
    const int st = tag_project(tc, lo, ext, x0, x1, y0, y1, ex, ey);
    bool all = (st & 1) != 0;
    const float m = VRT_TAG_MARGIN_PX;
    if (!all) {
        // off the screen by more than the margin AND more than its own error bound: nothing to tag, whatever the bound is
        const float gx = fmaxf(m, ex + 0.5f), gy = fmaxf(m, ey + 0.5f);
        if (x1 + gx < 0.0f || y1 + gy < 0.0f || x0 - gx > g.W || y0 - gy > g.H) return;
        if (st & 2) all = true;
    }
    int tx0 = (int)floorf(fmaxf(x0 - m, 0.0f) * 0.125f), tx1 = (int)floorf(fminf(x1 + m, g.W - 1.0f) * 0.125f);
    int ty0 = (int)floorf(fmaxf(y0 - m, 0.0f) * 0.125f), ty1 = (int)floorf(fminf(y1 + m, g.H - 1.0f) * 0.125f);
    if (!all && (tx1 - tx0 + 1) * (ty1 - ty0 + 1) > 1024) all = true;                           // (a cell that covers the screen: tagging it costs more than it saves)
    if (all) { tags[P.tags_per_frame - 1u] = P.tile_gen; return; }
    // screen row of blocks -> the row K1 finds it in: the launch's local rows (the strips this frame's rank owns), in dispatch
    // order (tile_origin: bottom rows first)
    const int nranks = P.sh.nranks, rows8 = P.sh.strip_rows >> 3, k = P.tile_h >> 3, T = P.tiles_y_local;
    if (nranks <= 1) {
        for (int ty = ty0; ty <= ty1; ty++) {
            const int tyl = ty / k;                                // the workgroup tile's local row, and the block's row within the tile
            if (tyl >= T) continue;
            const uint32_t row = (uint32_t)((T - 1 - tyl) * k + (ty - tyl * k));
            // (plain stores; looking first whether the block has its tag already -- most are covered by many cells -- measured slower)
            for (int tx = tx0; tx <= tx1; tx++) tags[row * P.tags_x + (uint32_t)tx] = P.tile_gen;
        }
        return;
    }
    // sharded: only the strips this frame's rank traces -- strip by strip, not row by row with a test (a rank of eight owns one
    // band of the screen: seven eighths of a cell's rows are somebody else's)
    const int s0 = ty0 / rows8, s1 = ty1 / rows8;
    int s = s0 + ((shard_rank - s0 % nranks) + nranks) % nranks;   // the first strip >= s0 that is dealt to shard_rank
    for (; s <= s1; s += nranks) {
        const int a = ty0 > s * rows8 ? ty0 : s * rows8, b = ty1 < (s + 1) * rows8 - 1 ? ty1 : (s + 1) * rows8 - 1;
        for (int ty = a; ty <= b; ty++) {
            const int local = (s / nranks) * rows8 + (ty - s * rows8);
            const int tyl = local / k;
            if (tyl >= T) continue;
            const uint32_t row = (uint32_t)((T - 1 - tyl) * k + (local - tyl * k));
            for (int tx = tx0; tx <= tx1; tx++) tags[row * P.tags_x + (uint32_t)tx] = P.tile_gen;
        }
    }
}

hipError_t launch_tile_tags(const GeomParams& p, hipStream_t s)
{
    if (p.n_cells == 0u) return hipSuccess;
    dim3 grid((p.n_cells + 255u) / 256u, (unsigned)p.n_frames), block(256);
    if (p.table) hipLaunchKernelGGL(k_tile_tags<true>, grid, block, 0, s, p);
    else         hipLaunchKernelGGL(k_tile_tags<false>, grid, block, 0, s, p);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Block verdicts: what a wave of the primary-only kernels does with its block -- trace it, store the miss pixel of its 8x8 pixels,
// or of two rows of its 32x8 span -- is a function of the block's tag, its span's, the frame's word and the frame's box rectangle
// (vrt_span.h).  One lane per block of every frame of the launch works it out, once, behind the tag kernel on the tag kernel's
// stream, and stores it as one byte (block_verdict_byte); K1's waves read the word their span's four bytes lie in.  The lanes of
// a 64 x 4 workgroup are 64 neighbouring blocks of four rows: their byte stores are whole 64-byte pieces of a row.
// ---------------------------------------------------------------------------------------------
// (table launches only: the slots are read from the table)
// vp: the launch's miss-colour planes (vrt_miss_plane.h) -- which of them each frame loads from goes into bits 2 - 4 of the bytes of
// the frame's blocks, and the planes' addresses into the VRT_VERDICT_HEAD bytes in front of the verdicts, where K1's sky waves find both
// without a kernel argument of their own.
__global__ __launch_bounds__(256) void k_block_verdicts(const GeomParams P, const VerdictPlanes vp)
{
    if (blockIdx.x == 0u && blockIdx.y == 0u && blockIdx.z == 0u && threadIdx.y == 0u && threadIdx.x < (uint32_t)VRT_SKY_PLANES)
        reinterpret_cast<const uint32_t**>(P.verdicts - VRT_VERDICT_HEAD)[threadIdx.x] = vp.plane[threadIdx.x];
    const uint32_t frame = blockIdx.z, col8 = blockIdx.x * 64u + threadIdx.x, row8 = blockIdx.y * 4u + threadIdx.y;
    const uint32_t k = (uint32_t)P.tile_h >> 3;                   // block rows per workgroup tile of K1 (1 or 2)
    const uint32_t blocks_x = (uint32_t)P.tiles_x * ((uint32_t)P.tile_w >> 3), blocks_y = (uint32_t)P.tiles_y_local * k;
    if (col8 >= blocks_x || row8 >= blocks_y) return;
    int shard_rank;
    uint32_t box;
    SlotOf<true>::rank_box(P, frame, shard_rank, box);
    // the block's first pixel row, as K1 finds it (tile_origin: tile rows in dispatch order, bottom rows first, strip by strip)
    const uint32_t tyl = row8 / k, t = (uint32_t)P.tiles_y_local - 1u - tyl;
    uint32_t strip_local = 0u, within = t;
    if (P.sh.nranks > 1) { strip_local = t / P.tps; within = t - strip_local * P.tps; }
    const uint32_t py0 = (strip_local * (uint32_t)P.sh.nranks + (uint32_t)shard_rank) * (uint32_t)P.sh.strip_rows + within * (uint32_t)P.tile_h + (row8 - tyl * k) * 8u;
    // the span's four tags (vrt_span.h verdict_tag: a launch without tags, columns the row does not have)
    const uint32_t* tg = P.tile_tags + (size_t)frame * P.tags_per_frame;
    const uint32_t gen = P.tile_gen, tags_x = P.tags_x, tag_all = tg[P.tags_per_frame - 1u];
    uint32_t tag[4];
#pragma unroll
    for (uint32_t j = 0; j < 4u; j++) tag[j] = verdict_tag(tg + row8 * tags_x, (col8 & ~3u) + j, tags_x, tag_all, gen);
    const bool span_path = (P.map.flags & VRT_MAPFLAG_SKY_SPAN) != 0u;
    P.verdicts[verdict_offset(row8, col8, frame, (uint32_t)P.n_frames, verdict_pitch(blocks_x))] =
        (uint8_t)(block_verdict_byte(tag[0], tag[1], tag[2], tag[3], col8, span_path, (uint32_t)P.W, tag_all, gen, box, py0) | ((uint32_t)vp.which[frame] << 2));
}

hipError_t launch_block_verdicts(const GeomParams& p, const VerdictPlanes& vp, hipStream_t s)
{
    const unsigned blocks_x = (unsigned)(p.tiles_x * (p.tile_w / 8)), blocks_y = (unsigned)(p.tiles_y_local * (p.tile_h / 8));
    if (!p.verdicts || blocks_x == 0u || blocks_y == 0u) return hipSuccess;
    if (!p.table) return hipErrorInvalidValue;
    dim3 grid((blocks_x + 63u) / 64u, (blocks_y + 3u) / 4u, (unsigned)p.n_frames), block(64, 4);
    hipLaunchKernelGGL(k_block_verdicts, grid, block, 0, s, p, vp);
    return hipGetLastError();
}

static int effective_traversal(int t, int fast_loop)
{
    if (t == VRT_TRAVERSAL_BRICK) return fast_loop == 2 ? VRT_TRAVERSAL_BRICK_CNT : t;
    if (fast_loop == 2 && (t == VRT_TRAVERSAL_AUTO || t == VRT_TRAVERSAL_DF)) return VRT_TRAVERSAL_DF_FAST_CNT;     // the loops' counting twins
    if (t == VRT_TRAVERSAL_DENSE || t == VRT_TRAVERSAL_BITMASK || t == VRT_TRAVERSAL_JUMP || t == VRT_TRAVERSAL_DFJ) return t;
    return fast_loop ? VRT_TRAVERSAL_DF_FAST : VRT_TRAVERSAL_DF;        // AUTO / DF
}

// K1's launcher and K2's for a launch's traversal: the one switch over the eleven (traversal, occ_in_lds) pairs
struct K1K2 { hipError_t (*primary)(const GeomParams&, hipStream_t); hipError_t (*shade)(const GeomParams&, hipStream_t); };
template <int TRAV, bool OCC_LDS> static K1K2 k1k2() { return {launch_primary_t<TRAV, OCC_LDS>, launch_shade_t<TRAV, OCC_LDS>}; }
static K1K2 launchers_of(const GeomParams& p)
{
    int t = effective_traversal((int)p.st.traversal, p.fast_loop);
    if (t == VRT_TRAVERSAL_DF_FAST) return k1k2<VRT_TRAVERSAL_DF_FAST, false>();
    if (t == VRT_TRAVERSAL_DF_FAST_CNT) return k1k2<VRT_TRAVERSAL_DF_FAST_CNT, false>();
    if (t == VRT_TRAVERSAL_BRICK) return k1k2<VRT_TRAVERSAL_BRICK, false>();
    if (t == VRT_TRAVERSAL_BRICK_CNT) return k1k2<VRT_TRAVERSAL_BRICK_CNT, false>();
    if (t == VRT_TRAVERSAL_DENSE) return k1k2<VRT_TRAVERSAL_DENSE, false>();
    if (t == VRT_TRAVERSAL_DF) return k1k2<VRT_TRAVERSAL_DF, false>();
    if (t == VRT_TRAVERSAL_DFJ) return k1k2<VRT_TRAVERSAL_DFJ, false>();
    if (t == VRT_TRAVERSAL_BITMASK) return p.occ_in_lds ? k1k2<VRT_TRAVERSAL_BITMASK, true>() : k1k2<VRT_TRAVERSAL_BITMASK, false>();
    return p.occ_in_lds ? k1k2<VRT_TRAVERSAL_JUMP, true>() : k1k2<VRT_TRAVERSAL_JUMP, false>();
}

hipError_t launch_primary(const GeomParams& p, hipStream_t s) { return launchers_of(p).primary(p, s); }
hipError_t launch_shade(const GeomParams& p, hipStream_t s) { return launchers_of(p).shade(p, s); }

const char* primary_kernel_name(int traversal, int fused, int occ_lds)
{
    int t = effective_traversal(traversal, 0);
    (void)fused; (void)occ_lds;
    return t == VRT_TRAVERSAL_DENSE ? "k_primary<dense>" : (t == VRT_TRAVERSAL_BITMASK ? "k_primary<bitmask>" : (t == VRT_TRAVERSAL_DF ? "k_primary<df>" : "k_primary<jump>"));
}

#endif // VRT_K1_PART == 0

} // namespace vrt
