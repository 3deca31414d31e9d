// vrt_march_fast.h -- DF_FAST: the four hand-written gfx950 look-up loops (df_fast_loop, df_prim_loop, df_any_loop,
// df_ao_pool_loop), trace_df_fast over them, and the AO ray pool in LDS (AoRay, AoLane, ao_ray_*, trace_ao_pool).
// Included by vrt_traverse.h.  Nearly all of it is inline assembly, device pass only; the host sees the structs and, at
// the end, empty stubs of the entry points.
#pragma once

#include "vrt_dda.h"     // (over vrt_volume.h: the data types and the DDA)

namespace vrt {

// an AO ray as df_ao_pool_loop takes it up (11 dwords; with its tag a column of 12), and the LDS bytes of a wave's pool + its two rows of counters
struct AoRay { float x, y, z, dx, dy, dz, gx, gy, gz; uint32_t idx0, voxoff; };
#define VRT_AO_SLOT 3840   // (dense scenes: 12 rows of 256 B + two rows of counters; brick scenes: 13 + 2)
// What a lane of the pool loop carries from one call to the next: the ray it is on (or the resting state it starts in)
struct AoLane { float x, y, z, dx, dy, dz, gx, gy, gz, cx, cy, cz; uint32_t idx0, voxoff, state, owner; };

#if defined(__HIP_DEVICE_COMPILE__)
// ---- DF, hand-written look-up loop (primary rays of the primary-only kernel) ----------------------------------------------
// Same march, same results as trace_df_impl<true, ., true>; what differs is what it costs to get from one look-up to the
// next.  Measured issue costs on gfx950 at 8 waves per SIMD (tools/ubench/issue_cost.hip; unit: one v_add_f32, about 3
// cycles of a SIMD): two-source vector ops 0.85-1.0, v_min3 / compares into a scalar pair / v_cndmask with a scalar mask /
// conversions / 24-bit mads about 1.5, a DPP step 1.2 (+0.4 for its s_nop), v_cmpx + v_add as a pair 1.7, scalar
// instructions issued between vector ones almost nothing.  So the loop is written for few, cheap VECTOR instructions:
//  * a finished lane does not leave EXEC: its deltas are zeroed (x + 0 = x: its sideDist stands still), its index points
//    at a byte that holds 0xFF, so the byte it reads IS its vote -- no select, no "done" mask, no live mask: every
//    iteration runs under the mask the loop was entered with;
//  * iterations are the EXEC-narrowing form (v_min3, then per axis v_cmpx + v_add under it: 6.9 units; the compare-
//    select-add form without EXEC writes measured 10.0);
//  * one compare (byte < 2) answers both "did a lane hit" and "is the run a single iteration" (half of all look-ups);
//    the DPP minimum runs only when every live lane has two or more iterations to go;
//  * where a ray stands is recovered from how far its sideDist has come since the START of the ray, n = rint(side * g + c)
//    per axis (c = -side0 * g): no copies of sideDist per run, no mapPos; the voxel id at a hit is read from a copy of
//    the volume in the fields' own layout at the same index.  |error of n| <= (n^2 + 3n) 2^-24 (n additions, each rounded to
//    the running sum's ulp), far below 1/2 for the budgets this path accepts (maxSteps <= 1024: 0.063).  An axis the ray
//    cannot step along has side = +inf and g = 0: the product is v_mul_legacy_f32's (0 * anything = 0; a NaN would
//    convert to INT_MIN, tools/ubench/nan_cvt.hip).
// Preconditions (checked by the host): v.df_fast, 1 <= maxSteps <= 1024.  The loop runs under the EXEC mask it is entered with.
// Hazards kept by hand inside the block (gfx950): a DPP source needs two wait states after a vector write, a DPP five
// after a write of EXEC; a scalar pair written by a vector compare needs two before a vector instruction reads it as mask.
// Counting twins of the three look-up loops (template CNT; vrt_render_geometry with VRT_FLAG_MARCHED_COUNTS / _LOOKUP_COUNTS): the same
// instructions plus a per-lane count of the clearance bytes a LIVE lane asks for (the index it loads from is not the 0xFF byte's)
// and of the voxel ids read at the end of a ray -- the bytes the march really requests, which bench.py reports next to the
// iterations it performs.  The product kernels are the CNT = false instantiations: not an instruction more.
#define VRT_CNT_LOOK "v_cmp_ne_u32_e32 vcc, %[sent], v53\n\t" "v_addc_co_u32_e32 %[lk], vcc, 0, %[lk], vcc\n\t"
#define VRT_CNT_FIND "v_add_u32 %[lk], 1, %[lk]\n\t"
#define VRT_CNT_OPND , [lk] "+v"(looks)
#define VRT_CNT_NONE
#define VRT_CNT_NOOP
template <bool CNT>
__device__ __forceinline__ void df_fast_loop(const uint8_t* base, uint32_t maxSteps, int pw, int pwh, uint32_t sentinel,
                                             float& x, float& y, float& z, float dx, float dy, float dz,
                                             float gx, float gy, float gz, float cx, float cy, float cz,
                                             uint32_t idx0, uint32_t voxoff, uint32_t& lmask, uint32_t& material, uint32_t& fetches,
                                             uint64_t kx, uint64_t ky, uint64_t kz, int incx, int incy, int incz, uint32_t anyhit, uint32_t pf, uint32_t& looks)
{
    // the same iteration that also moves the index of the lane's voxel: one more vector instruction per axis under the
    // EXEC mask that is there anyway -- cheaper than recovering the position afterwards for runs of up to four iterations
    // (three quarters of all runs)
#define VRT_F_EITER_IDX                                          \
        "s_mov_b64 exec, s[68:69]\n\t"                                  \
        "v_min3_u32 v48, %[x], %[y], %[z]\n\t"                    \
        "v_cmpx_eq_u32 v48, %[x]\n\t"                             \
        "v_add_f32 %[x], %[x], %[dx]\n\t"                         \
        "v_add_u32 v53, v53, %[ix]\n\t"                           \
        "s_mov_b64 exec, s[68:69]\n\t"                                  \
        "v_cmpx_eq_u32 v48, %[y]\n\t"                             \
        "v_add_f32 %[y], %[y], %[dy]\n\t"                         \
        "v_add_u32 v53, v53, %[iy]\n\t"                           \
        "s_mov_b64 exec, s[68:69]\n\t"                                  \
        "v_cmpx_eq_u32 v48, %[z]\n\t"                             \
        "v_add_f32 %[z], %[z], %[dz]\n\t"                         \
        "v_add_u32 v53, v53, %[iz]\n\t"
#define VRT_F_EITER                                              \
        "s_mov_b64 exec, s[68:69]\n\t"                                  \
        "v_min3_u32 v48, %[x], %[y], %[z]\n\t"                    \
        "v_cmpx_eq_u32 v48, %[x]\n\t"                             \
        "v_add_f32 %[x], %[x], %[dx]\n\t"                         \
        "s_mov_b64 exec, s[68:69]\n\t"                                  \
        "v_cmpx_eq_u32 v48, %[y]\n\t"                             \
        "v_add_f32 %[y], %[y], %[dy]\n\t"                         \
        "s_mov_b64 exec, s[68:69]\n\t"                                  \
        "v_cmpx_eq_u32 v48, %[z]\n\t"                             \
        "v_add_f32 %[z], %[z], %[dz]\n\t"
    // Secondary rays (pf != 0): with every look-up the bytes one step further along y and along z are asked for as well and
    // thrown away -- a ray creeping along a surface looks at memory after every iteration, each look a 64-lane gather that
    // comes from beyond the L2, and with a fifth of the pixels hitting there are no other waves to hide that behind; the next
    // cell of a single-iteration run is one of this cell's three neighbours (the one along x shares its cache line), so the
    // next look finds its line in the vector L1.  (Up to one row / slice past the fields' one-voxel border: the fields are
    // allocated with that much room around them and indexed from pwh bytes in front of field 0.)  The look-up's own load is
    // the oldest of the three: label 10 waits for all but the two youngest.
#define VRT_F_PREFETCH                                           \
        "s_cmp_eq_u32 %[pf], 0\n\t"                               \
        "s_cbranch_scc1 7f\n\t"                                   \
        "v_add_u32 v54, v53, %[iy]\n\t"                           \
        "global_load_ubyte v55, v54, %[base]\n\t"                 \
        "v_add_u32 v54, v53, %[iz]\n\t"                           \
        "global_load_ubyte v56, v54, %[base]\n\t"                 \
        "7:\n\t"
    // scalars of the block: s60 = i (iterations done by every live lane), s61 = kw, s62 = left / iterations still to do,
    // s63 = 0xFF, s[66:67] = saved EXEC; vectors: v48..v50 temporaries, v52 = the byte read = the lane's vote,
    // v53 = index of the byte to read next
    // the block starts on an instruction-cache line: where its loops fall relative to the lines is then a property of the block,
    // not of the code the compiler happens to put in front of it (6 % between two builds that differed elsewhere)
#define VRT_STR2(x) #x
#define VRT_STR(x) VRT_STR2(x)
#define VRT_F_LOOP(CNT_LOOK, CNT_FIND, CNT_OPND) \
    asm volatile( \
        ".p2align 6\n\t" \
        "s_mov_b32 s60, 0\n\t" \
        "s_movk_i32 s63, 0xff\n\t" \
 /* the loop runs under the EXEC mask it is entered with (all 64 lanes for primary rays; the hit lanes of a wave for its */ \
 /* secondary rays): no instruction here may write a lane outside it -- the compiler lets the registers of this block */ \
 /* hold live values of the OTHER lanes of a divergent branch (SIOptimizeVGPRLiveRange) */ \
        "s_mov_b64 s[68:69], exec\n\t" \
        "v_mov_b32 v53, %[idx0]\n\t" \
        "global_load_ubyte v52, v53, %[base]\n\t" \
        VRT_F_PREFETCH \
        "10:\n\t" /* ---- look-up: every lane's byte is here ---- */ \
        CNT_LOOK \
        "s_cmp_eq_u32 %[pf], 0\n\t" \
        "s_cbranch_scc1 8f\n\t" \
        "s_waitcnt vmcnt(2)\n\t" \
        "s_branch 11f\n\t" \
        "8:\n\t" \
        "s_waitcnt vmcnt(0)\n\t" \
        "11:\n\t" \
 /* any-hit rays (AO, shadow): a lane whose clearance covers what is left of its budget will test nothing but empty voxels */ \
 /* until the budget ends -- it is a miss with fetches = maxSteps, decided here without stepping (a 64-iteration AO ray */ \
 /* that starts in the open: by its first look-up; the fields hold clearances up to 127) */ \
        "s_cmp_eq_u32 %[any], 0\n\t" \
        "s_cbranch_scc1 111f\n\t" \
        "s_sub_u32 s62, %[maxs], s60\n\t" \
        "v_cmp_le_u32_e32 vcc, s62, v52\n\t" /* left <= clearance ... */ \
        "v_cmp_ne_u32_e64 s[64:65], s63, v52\n\t" /* ... of a lane that is still live */ \
        "s_and_b64 vcc, vcc, s[64:65]\n\t" \
        "s_cbranch_vccz 111f\n\t" \
        "s_and_saveexec_b64 s[66:67], vcc\n\t" \
        "s_cmp_eq_u32 %[any], 2\n\t" /* (any == 2: report the iterations taken, VolumeView::count_marched) */ \
        "s_cselect_b32 s62, s60, %[maxs]\n\t" \
        "v_mov_b32 %[fet], s62\n\t" \
        "v_mov_b32 %[dx], 0\n\t" \
        "v_mov_b32 %[dy], 0\n\t" \
        "v_mov_b32 %[dz], 0\n\t" \
        "v_mov_b32 %[gx], 0\n\t" \
        "v_mov_b32 %[gy], 0\n\t" \
        "v_mov_b32 %[gz], 0\n\t" \
        "v_mov_b32 %[cx], 0\n\t" \
        "v_mov_b32 %[cy], 0\n\t" \
        "v_mov_b32 %[cz], 0\n\t" \
        "v_mov_b32 %[ix], 0\n\t" \
        "v_mov_b32 %[iy], 0\n\t" \
        "v_mov_b32 %[iz], 0\n\t" \
        "v_mov_b32 %[idx0], %[sent]\n\t" \
        "v_mov_b32 v53, %[sent]\n\t" \
        "v_mov_b32 v52, s63\n\t" \
        "s_mov_b64 exec, s[66:67]\n\t" \
        "s_nop 4\n\t" \
        "111:\n\t" \
        "v_cmp_gt_u32_e32 vcc, 2, v52\n\t" /* 0 (solid / border) or 1 (single iteration) somewhere? */ \
        "s_cbranch_vccnz 15f\n\t" \
        "v_cmp_gt_u32_e32 vcc, 4, v52\n\t" /* 2 or 3 somewhere (and nothing below)? */ \
        "s_cbranch_vccnz 16f\n\t" \
        "s_cmp_eq_u64 s[68:69], -1\n\t" \
        "s_cbranch_scc0 14f\n\t" /* a partly filled wave: no DPP reduction (lane 63 may be off) */ \
        "v_mov_b32 v48, v52\n\t" /* wave minimum of the votes: every live lane has >= 4 */ \
        "s_nop 1\n\t" \
        "v_min_u32_dpp v48, v48, v48 row_shr:1 row_mask:0xf bank_mask:0xf\n\t" \
        "s_nop 1\n\t" \
        "v_min_u32_dpp v48, v48, v48 row_shr:2 row_mask:0xf bank_mask:0xf\n\t" \
        "s_nop 1\n\t" \
        "v_min_u32_dpp v48, v48, v48 row_shr:4 row_mask:0xf bank_mask:0xf\n\t" \
        "s_nop 1\n\t" \
        "v_min_u32_dpp v48, v48, v48 row_shr:8 row_mask:0xf bank_mask:0xf\n\t" \
        "s_nop 1\n\t" \
        "v_min_u32_dpp v48, v48, v48 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t" \
        "s_nop 1\n\t" \
        "v_min_u32_dpp v48, v48, v48 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t" \
        "s_sub_u32 s62, %[maxs], s60\n\t" /* left >= 1 */ \
        "s_nop 0\n\t" \
        "v_readlane_b32 s61, v48, 63\n\t" \
        "s_nop 1\n\t" \
        "s_cmp_eq_u32 s61, s63\n\t" \
        "s_cbranch_scc1 40f\n\t" /* nobody is live: done */ \
        "13:\n\t" \
        "s_min_u32 s61, s61, s62\n\t" \
        "s_cmp_le_u32 s61, 4\n\t" \
        "s_cbranch_scc1 18f\n\t" \
 /* ---- a run of kw = s61 >= 5 iterations: plain iterations, then the positions from the sideDist travelled ---- */ \
        "s_add_u32 s60, s60, s61\n\t" /* i += kw */ \
        "s_sub_u32 s62, s61, 1\n\t" /* plain iterations before the one whose masks are kept */ \
        "s_cmp_eq_u32 s62, 0\n\t" \
        "s_cbranch_scc1 34f\n\t" \
        "s_bitcmp0_b32 s62, 0\n\t" \
        "s_cbranch_scc1 31f\n\t" \
        VRT_F_EITER \
        "31:\n\t" \
        "s_bitcmp0_b32 s62, 1\n\t" \
        "s_cbranch_scc1 32f\n\t" \
        VRT_F_EITER \
        VRT_F_EITER \
        "32:\n\t" \
        "s_lshr_b32 s62, s62, 2\n\t" /* quads; SCC = (quads != 0) */ \
        "s_cbranch_scc0 34f\n\t" \
        "s_sub_u32 s62, s62, 1\n\t" \
        "33:\n\t" \
        VRT_F_EITER \
        VRT_F_EITER \
        VRT_F_EITER \
        VRT_F_EITER \
        "s_sub_u32 s62, s62, 1\n\t" /* SCC = borrow: that was the last quad */ \
        "s_cbranch_scc0 33b\n\t" \
        "34:\n\t" /* the run's last iteration: its EXEC masks are the mask bits */ \
        "s_mov_b64 exec, s[68:69]\n\t" \
        "v_min3_u32 v48, %[x], %[y], %[z]\n\t" \
        "v_cmpx_eq_u32 v48, %[x]\n\t" \
        "s_mov_b64 %[kx], exec\n\t" \
        "v_add_f32 %[x], %[x], %[dx]\n\t" \
        "s_mov_b64 exec, s[68:69]\n\t" \
        "v_cmpx_eq_u32 v48, %[y]\n\t" \
        "s_mov_b64 %[ky], exec\n\t" \
        "v_add_f32 %[y], %[y], %[dy]\n\t" \
        "s_mov_b64 exec, s[68:69]\n\t" \
        "v_cmpx_eq_u32 v48, %[z]\n\t" \
        "s_mov_b64 %[kz], exec\n\t" \
        "v_add_f32 %[z], %[z], %[dz]\n\t" \
        "s_mov_b64 exec, s[68:69]\n\t" \
 /* ---- where is every lane now?  request its next byte ---- */ \
        "v_mul_legacy_f32 v48, %[x], %[gx]\n\t" /* (legacy: inf * 0 = 0, an axis the ray cannot step along) */ \
        "v_mul_legacy_f32 v49, %[y], %[gy]\n\t" \
        "v_mul_legacy_f32 v50, %[z], %[gz]\n\t" \
        "v_add_f32 v48, v48, %[cx]\n\t" \
        "v_add_f32 v49, v49, %[cy]\n\t" \
        "v_add_f32 v50, v50, %[cz]\n\t" \
        "v_cvt_rpi_i32_f32 v48, v48\n\t" \
        "v_cvt_rpi_i32_f32 v49, v49\n\t" \
        "v_cvt_rpi_i32_f32 v50, v50\n\t" \
        "v_mad_i32_i24 v48, v49, %[pw], v48\n\t" \
        "v_mad_i32_i24 v48, v50, %[pwh], v48\n\t" \
        "v_add_u32 v53, %[idx0], v48\n\t" \
        "global_load_ubyte v52, v53, %[base]\n\t" \
        VRT_F_PREFETCH \
        "s_cmp_lt_u32 s60, %[maxs]\n\t" \
        "s_cbranch_scc1 10b\n\t" \
 /* ---- the budget is spent: the lanes that are still live (their start index is not the 0xFF byte's) stop here ---- */ \
        "19:\n\t" \
        "v_cmp_ne_u32_e32 vcc, %[sent], %[idx0]\n\t" \
        "s_and_saveexec_b64 s[66:67], vcc\n\t" \
        "v_cndmask_b32_e64 v48, 0, 1, %[kx]\n\t" \
        "v_cndmask_b32_e64 v49, 0, 2, %[ky]\n\t" \
        "v_cndmask_b32_e64 v50, 0, 4, %[kz]\n\t" \
        "v_or3_b32 %[lm], v48, v49, v50\n\t" \
        "v_mov_b32 %[fet], s60\n\t" \
        "s_mov_b64 exec, s[66:67]\n\t" \
        "s_branch 40f\n\t" \
        "14:\n\t" /* ---- minimum of a partly filled wave: binary search by votes ---- */ \
        "v_cmp_ne_u32_e32 vcc, s63, v52\n\t" \
        "s_cbranch_vccz 40f\n\t" /* nobody is live: done */ \
        "v_min_u32 v48, 63, v52\n\t" /* (a finished lane: 63, never below a live one) */ \
        "s_sub_u32 s62, %[maxs], s60\n\t" \
        "s_mov_b32 s61, 0\n\t" \
        "s_or_b32 s66, s61, 32\n\t" \
        "v_cmp_gt_u32_e32 vcc, s66, v48\n\t" \
        "s_cmp_eq_u64 vcc, 0\n\t" \
        "s_cselect_b32 s61, s66, s61\n\t" \
        "s_or_b32 s66, s61, 16\n\t" \
        "v_cmp_gt_u32_e32 vcc, s66, v48\n\t" \
        "s_cmp_eq_u64 vcc, 0\n\t" \
        "s_cselect_b32 s61, s66, s61\n\t" \
        "s_or_b32 s66, s61, 8\n\t" \
        "v_cmp_gt_u32_e32 vcc, s66, v48\n\t" \
        "s_cmp_eq_u64 vcc, 0\n\t" \
        "s_cselect_b32 s61, s66, s61\n\t" \
        "s_or_b32 s66, s61, 4\n\t" \
        "v_cmp_gt_u32_e32 vcc, s66, v48\n\t" \
        "s_cmp_eq_u64 vcc, 0\n\t" \
        "s_cselect_b32 s61, s66, s61\n\t" \
        "s_or_b32 s66, s61, 2\n\t" \
        "v_cmp_gt_u32_e32 vcc, s66, v48\n\t" \
        "s_cmp_eq_u64 vcc, 0\n\t" \
        "s_cselect_b32 s61, s66, s61\n\t" \
        "s_or_b32 s66, s61, 1\n\t" \
        "v_cmp_gt_u32_e32 vcc, s66, v48\n\t" \
        "s_cmp_eq_u64 vcc, 0\n\t" \
        "s_cselect_b32 s61, s66, s61\n\t" \
        "s_branch 13b\n\t" \
        "16:\n\t" /* ---- the smallest vote is 2 or 3 ---- */ \
        "v_cmp_eq_u32_e32 vcc, 2, v52\n\t" \
        "s_sub_u32 s62, %[maxs], s60\n\t" \
        "s_mov_b32 s61, 3\n\t" \
        "s_cbranch_vccz 17f\n\t" \
        "s_mov_b32 s61, 2\n\t" \
        "17:\n\t" \
        "s_min_u32 s61, s61, s62\n\t" \
        "18:\n\t" /* ---- a run of kw = s61 in 1..4 iterations, index moved along ---- */ \
        "s_add_u32 s60, s60, s61\n\t" \
        "s_cmp_eq_u32 s61, 1\n\t" \
        "s_cbranch_scc1 184f\n\t" \
        "s_cmp_eq_u32 s61, 2\n\t" \
        "s_cbranch_scc1 183f\n\t" \
        "s_cmp_eq_u32 s61, 3\n\t" \
        "s_cbranch_scc1 182f\n\t" \
        VRT_F_EITER_IDX \
        "182:\n\t" \
        VRT_F_EITER_IDX \
        "183:\n\t" \
        VRT_F_EITER_IDX \
        "184:\n\t" \
        "s_mov_b64 exec, s[68:69]\n\t" \
        "v_min3_u32 v48, %[x], %[y], %[z]\n\t" \
        "v_cmpx_eq_u32 v48, %[x]\n\t" \
        "s_mov_b64 %[kx], exec\n\t" \
        "v_add_f32 %[x], %[x], %[dx]\n\t" \
        "v_add_u32 v53, v53, %[ix]\n\t" \
        "s_mov_b64 exec, s[68:69]\n\t" \
        "v_cmpx_eq_u32 v48, %[y]\n\t" \
        "s_mov_b64 %[ky], exec\n\t" \
        "v_add_f32 %[y], %[y], %[dy]\n\t" \
        "v_add_u32 v53, v53, %[iy]\n\t" \
        "s_mov_b64 exec, s[68:69]\n\t" \
        "v_cmpx_eq_u32 v48, %[z]\n\t" \
        "s_mov_b64 %[kz], exec\n\t" \
        "v_add_f32 %[z], %[z], %[dz]\n\t" \
        "v_add_u32 v53, v53, %[iz]\n\t" \
        "s_mov_b64 exec, s[68:69]\n\t" \
        "global_load_ubyte v52, v53, %[base]\n\t" \
        VRT_F_PREFETCH \
        "s_cmp_lt_u32 s60, %[maxs]\n\t" \
        "s_cbranch_scc1 10b\n\t" \
        "s_branch 19b\n\t" \
        "15:\n\t" /* ---- some lane read 0 or 1 ---- */ \
        "v_cmp_eq_u32_e32 vcc, 0, v52\n\t" \
        "s_mov_b32 s61, 1\n\t" \
        "s_cbranch_vccz 18b\n\t" /* only 1s: a single-iteration run */ \
        "s_and_saveexec_b64 s[66:67], vcc\n\t" /* lanes that read 0: a solid voxel, or the border */ \
        CNT_FIND \
        "v_add_u32 v48, v53, %[voxoff]\n\t" \
        "global_load_ubyte %[mat], v48, %[base]\n\t" /* the voxel id (0 in the border: the ray has left the volume) */ \
        "v_cndmask_b32_e64 v48, 0, 1, %[kx]\n\t" \
        "v_cndmask_b32_e64 v49, 0, 2, %[ky]\n\t" \
        "v_cndmask_b32_e64 v50, 0, 4, %[kz]\n\t" \
        "v_or3_b32 %[lm], v48, v49, v50\n\t" \
        "v_mov_b32 %[fet], s60\n\t" \
        "v_mov_b32 %[dx], 0\n\t" \
        "v_mov_b32 %[dy], 0\n\t" \
        "v_mov_b32 %[dz], 0\n\t" \
        "v_mov_b32 %[gx], 0\n\t" \
        "v_mov_b32 %[gy], 0\n\t" \
        "v_mov_b32 %[gz], 0\n\t" \
        "v_mov_b32 %[cx], 0\n\t" \
        "v_mov_b32 %[cy], 0\n\t" \
        "v_mov_b32 %[cz], 0\n\t" \
        "v_mov_b32 %[ix], 0\n\t" \
        "v_mov_b32 %[iy], 0\n\t" \
        "v_mov_b32 %[iz], 0\n\t" \
        "v_mov_b32 %[idx0], %[sent]\n\t" \
        "v_mov_b32 v53, %[sent]\n\t" \
        "v_mov_b32 v52, s63\n\t" \
        "s_mov_b64 exec, s[66:67]\n\t" \
        "s_nop 4\n\t" /* EXEC written -> DPP: five wait states */ \
        "s_branch 11b\n\t" /* the other lanes' bytes are still to be looked at */ \
        "40:\n\t" \
        "s_waitcnt vmcnt(0)\n\t" \
        "s_mov_b64 exec, s[68:69]\n\t" \
        : [x] "+v"(x), [y] "+v"(y), [z] "+v"(z), [dx] "+v"(dx), [dy] "+v"(dy), [dz] "+v"(dz), \
          [gx] "+v"(gx), [gy] "+v"(gy), [gz] "+v"(gz), [cx] "+v"(cx), [cy] "+v"(cy), [cz] "+v"(cz), \
          [idx0] "+v"(idx0), [lm] "+v"(lmask), [mat] "+v"(material), [fet] "+v"(fetches), \
          [kx] "+s"(kx), [ky] "+s"(ky), [kz] "+s"(kz), [ix] "+v"(incx), [iy] "+v"(incy), [iz] "+v"(incz) CNT_OPND \
        : [voxoff] "v"(voxoff), [base] "s"(base), [maxs] "s"(maxSteps), [pw] "s"(pw), [pwh] "s"(pwh), [sent] "s"(sentinel), [any] "s"(anyhit), [pf] "s"(pf) \
        : "vcc", "scc", "memory", "v48", "v49", "v50", "v52", "v53", "v54", "v55", "v56", \
          "s60", "s61", "s62", "s63", "s64", "s65", "s66", "s67", "s68", "s69")
    if (CNT) { VRT_F_LOOP(VRT_CNT_LOOK, VRT_CNT_FIND, VRT_CNT_OPND); }
    else { VRT_F_LOOP(VRT_CNT_NONE, VRT_CNT_NONE, VRT_CNT_NOOP); }
#undef VRT_F_EITER
#undef VRT_F_EITER_IDX
#undef VRT_F_PREFETCH
}

// ---- the same march for PRIMARY rays: long runs by threshold, every lane its own clearance ------------------------------------
// sideDist of an axis only ever grows by that axis' own additions, x (+) dx (+) dx ..., whatever the other two axes do: the three
// axes are three independent sequences, and the shader's loop is their MERGE -- every iteration takes the smallest value (equal
// values together, frag:164).  So "the state after every event with a value <= T has been processed" is a state the loop passes
// through, for ANY T, and it can be reached without merging: step each axis on its own while its sideDist is <= T.  One
// compare and one addition per STEP (v_cmpx narrows EXEC monotonically: a lane that has passed T stays out, nothing to put back
// between steps) where the merged iteration spends seven vector and three scalar instructions on the same addition.  T is the
// lane's own: with clearance c every position at most c - 1 steps away along each axis lies in the empty cube, and
//     T = min over axes of (side + (c - 1) delta), times (1 - 2^-16),
// is below the value at which any axis would take its c-th step (c - 1 <= 126 roundings of 2^-24 each cannot bridge 2^-16), so a
// lane spends ITS OWN clearance and the wave needs no vote on the run length at all.  The position afterwards follows from the
// sideDist travelled, as in df_fast_loop's long runs; the cell a lane lands on lies inside the cube, i.e. it is EMPTY: a solid
// voxel is only ever found after one of the short runs (a vote of 1..4 somewhere in the wave: up to four merged iterations for
// everybody, as before), which leave the mask bits of their last iteration behind.
// What this loop does not know is how many ITERATIONS a lane has taken (two axes that hold the same value step in one): it has
// no budget.  So it is entered only by waves none of whose rays can reach the budget at all (trace_df_fast): a ray takes at most
// one step per integer plane it crosses, i.e. no more than (its length inside the box) x (|dir.x| + |dir.y| + |dir.z|) + 3
// iterations whatever it meets; where that bound stays below maxSteps the budget is dead code, and every other wave takes
// df_fast_loop, which counts.  A ray that finds nothing leaves through the border or an open cell as it always did.  Launches
// that report iteration counts do not come here.
// Hazards as in df_fast_loop.  Runs under the EXEC mask it is entered with.
template <bool CNT>
__device__ __forceinline__ void df_prim_loop(const uint8_t* base, int pw, int pwh, uint32_t sentinel,
                                             float& x, float& y, float& z, float dx, float dy, float dz,
                                             float gx, float gy, float gz, float cx, float cy, float cz,
                                             uint32_t idx0, uint32_t voxoff, uint32_t& lmask, uint32_t& material,
                                             uint64_t kx, uint64_t ky, uint64_t kz, int incx, int incy, int incz, uint32_t& looks)
{
#define VRT_P_EITER_IDX                                          \
        "s_mov_b64 exec, s[68:69]\n\t"                            \
        "v_min3_u32 v48, %[x], %[y], %[z]\n\t"                    \
        "v_cmpx_eq_u32 v48, %[x]\n\t"                             \
        "v_add_f32 %[x], %[x], %[dx]\n\t"                         \
        "v_add_u32 v53, v53, %[ix]\n\t"                           \
        "s_mov_b64 exec, s[68:69]\n\t"                            \
        "v_cmpx_eq_u32 v48, %[y]\n\t"                             \
        "v_add_f32 %[y], %[y], %[dy]\n\t"                         \
        "v_add_u32 v53, v53, %[iy]\n\t"                           \
        "s_mov_b64 exec, s[68:69]\n\t"                            \
        "v_cmpx_eq_u32 v48, %[z]\n\t"                             \
        "v_add_f32 %[z], %[z], %[dz]\n\t"                         \
        "v_add_u32 v53, v53, %[iz]\n\t"
    // one axis of a threshold run: up to 128 steps, four per trip; EXEC only ever narrows, so the trip that empties it ends the axis
#define VRT_P_AXIS(A, DA, L)                                     \
        "s_movk_i32 s61, 31\n\t"                                  \
        L "0:\n\t"                                                \
        "v_cmpx_ge_f32 v54, " A "\n\t"                        \
        "v_add_f32 " A ", " A ", " DA "\n\t"                      \
        "v_cmpx_ge_f32 v54, " A "\n\t"                        \
        "v_add_f32 " A ", " A ", " DA "\n\t"                      \
        "v_cmpx_ge_f32 v54, " A "\n\t"                        \
        "v_add_f32 " A ", " A ", " DA "\n\t"                      \
        "v_cmpx_ge_f32 v54, " A "\n\t"                        \
        "v_add_f32 " A ", " A ", " DA "\n\t"                      \
        "s_cbranch_execz " L "1f\n\t"                             \
        "s_sub_u32 s61, s61, 1\n\t"                               \
        "s_cbranch_scc0 " L "0b\n\t"                              \
        L "1:\n\t"                                                \
        "s_mov_b64 exec, s[68:69]\n\t"
    // scalars of the block: s61 = run length / trip counter, s63 = 0xFF, s[66:67] = saved EXEC, s[68:69] = EXEC on entry;
    // vectors: v48..v50 temporaries, v52 = the byte read (the lane's clearance; 0xFF: finished), v53 = index of the byte to
    // read next, v54 = the lane's threshold
#define VRT_P_LOOP(CNT_LOOK, CNT_FIND, CNT_OPND) \
    asm volatile( \
        ".p2align 6\n\t" \
        "s_movk_i32 s63, 0xff\n\t" \
        "s_mov_b64 s[68:69], exec\n\t" \
        "v_mov_b32 v53, %[idx0]\n\t" \
        "s_mov_b32 s62, 0\n\t" \
        "global_load_ubyte v52, v53, %[base]\n\t" \
        "10:\n\t" /* ---- look-up: every lane's byte is here ---- */ \
        CNT_LOOK \
 /* (every look-up is followed by at least one step of every live lane, and no ray has more than 3 x 1024 steps in it: the */ \
 /* count below only ends a wave whose rays cannot step at all -- direction (0, 0, 0): the shader's loop spins to its budget */ \
 /* and misses, and so does a lane that is still live here) */ \
        "s_add_u32 s62, s62, 1\n\t" \
        "s_cmp_gt_u32 s62, 0x1000\n\t" \
        "s_cbranch_scc1 40f\n\t" \
        "s_waitcnt vmcnt(0)\n\t" \
        "11:\n\t" \
        "v_cmp_gt_u32_e32 vcc, 2, v52\n\t" /* 0 (solid / border / open) or 1 somewhere? */ \
        "s_cbranch_vccnz 15f\n\t" \
        "v_cmp_gt_u32_e32 vcc, 5, v52\n\t" /* 2, 3 or 4 somewhere (and nothing below)? */ \
        "s_cbranch_vccnz 16f\n\t" \
        "v_cmp_ne_u32_e32 vcc, s63, v52\n\t" /* everybody has >= 5, or is finished -- anybody live at all? */ \
        "s_cbranch_vccz 40f\n\t" \
 /* ---- a threshold run: T = min(side + (c - 1) delta) (1 - 2^-16); a finished lane (delta 0, c - 1 = 254) gets T below */ \
 /* every side and takes no step; an axis that cannot step has side = delta = inf and never holds the minimum ---- */ \
        "v_add_u32 v48, -1, v52\n\t" \
        "v_cvt_f32_u32_e32 v48, v48\n\t" \
        "v_fma_f32 v49, v48, %[dx], %[x]\n\t" \
        "v_fma_f32 v50, v48, %[dy], %[y]\n\t" \
        "v_fma_f32 v48, v48, %[dz], %[z]\n\t" \
        "v_min3_f32 v49, v49, v50, v48\n\t" \
        "v_mul_f32 v54, 0x3f7fff00, v49\n\t" \
        VRT_P_AXIS("%[x]", "%[dx]", "2") \
        VRT_P_AXIS("%[y]", "%[dy]", "3") \
        VRT_P_AXIS("%[z]", "%[dz]", "5") \
 /* ---- where is every lane now?  request its next byte ---- */ \
        "v_mul_legacy_f32 v48, %[x], %[gx]\n\t" /* (legacy: inf * 0 = 0, an axis the ray cannot step along) */ \
        "v_mul_legacy_f32 v49, %[y], %[gy]\n\t" \
        "v_mul_legacy_f32 v50, %[z], %[gz]\n\t" \
        "v_add_f32 v48, v48, %[cx]\n\t" \
        "v_add_f32 v49, v49, %[cy]\n\t" \
        "v_add_f32 v50, v50, %[cz]\n\t" \
        "v_cvt_rpi_i32_f32 v48, v48\n\t" \
        "v_cvt_rpi_i32_f32 v49, v49\n\t" \
        "v_cvt_rpi_i32_f32 v50, v50\n\t" \
        "v_mad_i32_i24 v48, v49, %[pw], v48\n\t" \
        "v_mad_i32_i24 v48, v50, %[pwh], v48\n\t" \
        "v_add_u32 v53, %[idx0], v48\n\t" \
        "global_load_ubyte v52, v53, %[base]\n\t" \
        "s_branch 10b\n\t" \
        "16:\n\t" /* ---- the smallest vote is 2, 3 or 4 ---- */ \
        "v_cmp_eq_u32_e32 vcc, 2, v52\n\t" \
        "s_mov_b32 s61, 2\n\t" \
        "s_cbranch_vccnz 18f\n\t" \
        "v_cmp_eq_u32_e32 vcc, 3, v52\n\t" \
        "s_mov_b32 s61, 3\n\t" \
        "s_cbranch_vccnz 18f\n\t" \
        "s_mov_b32 s61, 4\n\t" \
        "18:\n\t" /* ---- a run of s61 in 1..4 merged iterations, index moved along ---- */ \
        "s_cmp_eq_u32 s61, 1\n\t" \
        "s_cbranch_scc1 184f\n\t" \
        "s_cmp_eq_u32 s61, 2\n\t" \
        "s_cbranch_scc1 183f\n\t" \
        "s_cmp_eq_u32 s61, 3\n\t" \
        "s_cbranch_scc1 182f\n\t" \
        VRT_P_EITER_IDX \
        "182:\n\t" \
        VRT_P_EITER_IDX \
        "183:\n\t" \
        VRT_P_EITER_IDX \
        "184:\n\t" \
        "s_mov_b64 exec, s[68:69]\n\t" \
        "v_min3_u32 v48, %[x], %[y], %[z]\n\t" \
        "v_cmpx_eq_u32 v48, %[x]\n\t" \
        "s_mov_b64 %[kx], exec\n\t" \
        "v_add_f32 %[x], %[x], %[dx]\n\t" \
        "v_add_u32 v53, v53, %[ix]\n\t" \
        "s_mov_b64 exec, s[68:69]\n\t" \
        "v_cmpx_eq_u32 v48, %[y]\n\t" \
        "s_mov_b64 %[ky], exec\n\t" \
        "v_add_f32 %[y], %[y], %[dy]\n\t" \
        "v_add_u32 v53, v53, %[iy]\n\t" \
        "s_mov_b64 exec, s[68:69]\n\t" \
        "v_cmpx_eq_u32 v48, %[z]\n\t" \
        "s_mov_b64 %[kz], exec\n\t" \
        "v_add_f32 %[z], %[z], %[dz]\n\t" \
        "v_add_u32 v53, v53, %[iz]\n\t" \
        "s_mov_b64 exec, s[68:69]\n\t" \
        "global_load_ubyte v52, v53, %[base]\n\t" \
        "s_branch 10b\n\t" \
        "15:\n\t" /* ---- some lane read 0 or 1 ---- */ \
        "v_cmp_eq_u32_e32 vcc, 0, v52\n\t" \
        "s_mov_b32 s61, 1\n\t" \
        "s_cbranch_vccz 18b\n\t" /* only 1s: a single-iteration run */ \
        "s_and_saveexec_b64 s[66:67], vcc\n\t" /* lanes that read 0: a solid voxel, the border, or an open cell */ \
        CNT_FIND \
        "v_add_u32 v48, v53, %[voxoff]\n\t" \
        "global_load_ubyte %[mat], v48, %[base]\n\t" /* the voxel id (0 in the border and in an open cell: a miss) */ \
        "v_cndmask_b32_e64 v48, 0, 1, %[kx]\n\t" \
        "v_cndmask_b32_e64 v49, 0, 2, %[ky]\n\t" \
        "v_cndmask_b32_e64 v50, 0, 4, %[kz]\n\t" \
        "v_or3_b32 %[lm], v48, v49, v50\n\t" \
        "v_mov_b32 %[dx], 0\n\t" \
        "v_mov_b32 %[dy], 0\n\t" \
        "v_mov_b32 %[dz], 0\n\t" \
        "v_mov_b32 %[gx], 0\n\t" \
        "v_mov_b32 %[gy], 0\n\t" \
        "v_mov_b32 %[gz], 0\n\t" \
        "v_mov_b32 %[cx], 0\n\t" \
        "v_mov_b32 %[cy], 0\n\t" \
        "v_mov_b32 %[cz], 0\n\t" \
        "v_mov_b32 %[ix], 0\n\t" \
        "v_mov_b32 %[iy], 0\n\t" \
        "v_mov_b32 %[iz], 0\n\t" \
        "v_mov_b32 %[idx0], %[sent]\n\t" \
        "v_mov_b32 v53, %[sent]\n\t" \
        "v_mov_b32 v52, s63\n\t" \
        "s_mov_b64 exec, s[66:67]\n\t" \
        "s_branch 11b\n\t" /* the other lanes' bytes are still to be looked at */ \
        "40:\n\t" \
        "s_waitcnt vmcnt(0)\n\t" \
        "s_mov_b64 exec, s[68:69]\n\t" \
        : [x] "+v"(x), [y] "+v"(y), [z] "+v"(z), [dx] "+v"(dx), [dy] "+v"(dy), [dz] "+v"(dz), \
          [gx] "+v"(gx), [gy] "+v"(gy), [gz] "+v"(gz), [cx] "+v"(cx), [cy] "+v"(cy), [cz] "+v"(cz), \
          [idx0] "+v"(idx0), [lm] "+v"(lmask), [mat] "+v"(material), \
          [kx] "+s"(kx), [ky] "+s"(ky), [kz] "+s"(kz), [ix] "+v"(incx), [iy] "+v"(incy), [iz] "+v"(incz) CNT_OPND \
        : [voxoff] "v"(voxoff), [base] "s"(base), [pw] "s"(pw), [pwh] "s"(pwh), [sent] "s"(sentinel) \
        : "vcc", "scc", "memory", "v48", "v49", "v50", "v52", "v53", "v54", \
          "s61", "s62", "s63", "s66", "s67", "s68", "s69")
    if (CNT) { VRT_P_LOOP(VRT_CNT_LOOK, VRT_CNT_FIND, VRT_CNT_OPND); }
    else { VRT_P_LOOP(VRT_CNT_NONE, VRT_CNT_NONE, VRT_CNT_NOOP); }
#undef VRT_P_AXIS
#undef VRT_P_EITER_IDX
}

// ---- the same march for rays that point every way (AO): every lane spends ITS OWN clearance -------------------------------
// The lanes of a primary or a shadow wave are neighbours going the same way, and the wave-wide minimum of their clearances
// costs little.  The AO rays of a wave point every way from a surface: somebody's cube is always tiny, the minimum is 1 or 2, and
// the wave looks at memory -- a gather of 64 unrelated cache lines -- after every iteration or two.  Here a lane that read
// clearance c takes c iterations of its own while the others take theirs (an iteration runs under the mask of the lanes that
// still have some left: one compare and one subtraction more than the 7 instructions of the plain one), and the wave looks
// again only when everybody has used his up: the number of looks is the number the NEEDIEST lane needs, not the sum over the
// minima.  Positions from the sideDist travelled, as in the long runs of df_fast_loop.  Any-hit rays only: no mask bits, no
// per-lane iteration of a hit to remember -- a lane's own iteration count (fetches) is its i.
// Same fp32 additions per lane, in the same order: bit-identical results.  Runs under the EXEC mask it is entered with.
#ifndef VRT_OWN_CAP
#define VRT_OWN_CAP 6                // iterations of its own a lane may take per look.  Round 3 (df_any_loop, a ray per lane): 4.  With the wave's pool
                                     // (df_ao_pool_loop) a lane that is done does not wait for the others, so longer stretches pay: reference defaults /
                                     // Mandelbulb 4K at 3: 138 us / 1.09 ms, 4: 128 / 1.06, 6: 121 / 1.025, 8: 118 / 1.047, 12: 120 / 1.065, 16: 126 / 1.10
#endif
template <bool CNT>
__device__ __forceinline__ void df_any_loop(const uint8_t* base, uint32_t maxSteps, int pw, int pwh, uint32_t sentinel,
                                            float& x, float& y, float& z, float dx, float dy, float dz,
                                            float gx, float gy, float gz, float cx, float cy, float cz,
                                            uint32_t idx0, uint32_t voxoff, uint32_t& material, uint32_t& fetches, uint32_t marched, uint32_t& looks)
{
    // vectors of the block: v48..v50 temporaries, v52 the byte read, v53 its index, v54 = i (iterations this lane has taken),
    // v55 = iterations this lane may still take before it has to look again; scalars: s63 = 0xFF, s[64:65] lanes with some left,
    // s[66:67] saved EXEC, s[68:69] EXEC on entry
#define VRT_A_ITER                                               \
        "v_cmp_lt_u32_e32 vcc, 0, v55\n\t"                        \
        "s_cbranch_vccz 30f\n\t"                                  \
        "s_mov_b64 s[64:65], vcc\n\t"                             \
        "s_mov_b64 exec, vcc\n\t"                                 \
        "v_subrev_u32 v55, 1, v55\n\t"                            \
        "v_min3_u32 v48, %[x], %[y], %[z]\n\t"                    \
        "v_cmpx_eq_u32 v48, %[x]\n\t"                             \
        "v_add_f32 %[x], %[x], %[dx]\n\t"                         \
        "s_mov_b64 exec, s[64:65]\n\t"                            \
        "v_cmpx_eq_u32 v48, %[y]\n\t"                             \
        "v_add_f32 %[y], %[y], %[dy]\n\t"                         \
        "s_mov_b64 exec, s[64:65]\n\t"                            \
        "v_cmpx_eq_u32 v48, %[z]\n\t"                             \
        "v_add_f32 %[z], %[z], %[dz]\n\t"                         \
        "s_mov_b64 exec, s[68:69]\n\t"
#define VRT_A_FINISH                                             \
        "v_mov_b32 %[dx], 0\n\t"                                  \
        "v_mov_b32 %[dy], 0\n\t"                                  \
        "v_mov_b32 %[dz], 0\n\t"                                  \
        "v_mov_b32 %[gx], 0\n\t"                                  \
        "v_mov_b32 %[gy], 0\n\t"                                  \
        "v_mov_b32 %[gz], 0\n\t"                                  \
        "v_mov_b32 %[cx], 0\n\t"                                  \
        "v_mov_b32 %[cy], 0\n\t"                                  \
        "v_mov_b32 %[cz], 0\n\t"                                  \
        "v_mov_b32 %[idx0], %[sent]\n\t"                          \
        "v_mov_b32 v53, %[sent]\n\t"                              \
        "v_mov_b32 v52, s63\n\t"
#define VRT_A_LOOP(CNT_LOOK, CNT_FIND, CNT_OPND) \
    asm volatile( \
        ".p2align 6\n\t" \
        "s_movk_i32 s63, 0xff\n\t" \
        "s_mov_b64 s[68:69], exec\n\t" \
        "v_mov_b32 v53, %[idx0]\n\t" \
        "v_mov_b32 v54, 0\n\t" \
        "global_load_ubyte v52, v53, %[base]\n\t" \
        "10:\n\t" /* ---- every lane's byte is here ---- */ \
        CNT_LOOK \
        "s_waitcnt vmcnt(0)\n\t" \
        "v_cmp_eq_u32_e32 vcc, 0, v52\n\t" /* solid, border or open cell: the lane ends here */ \
        "s_cbranch_vccz 12f\n\t" \
        "s_and_saveexec_b64 s[66:67], vcc\n\t" \
        "v_add_u32 v48, v53, %[voxoff]\n\t" \
        CNT_FIND \
        "global_load_ubyte %[mat], v48, %[base]\n\t" /* the voxel id says which */ \
        "v_mov_b32 %[fet], v54\n\t" \
        VRT_A_FINISH \
        "s_mov_b64 exec, s[66:67]\n\t" \
        "12:\n\t" \
        "v_cmp_ne_u32_e64 s[64:65], s63, v52\n\t" /* live lanes ... */ \
        "v_sub_u32 v48, %[maxs], v54\n\t" /* ... what is left of their budget ... */ \
        "s_nop 0\n\t" \
        "v_cmp_le_u32_e32 vcc, v48, v52\n\t" /* ... and whether the clearance covers it: a miss at the budget */ \
        "s_and_b64 vcc, vcc, s[64:65]\n\t" \
        "s_cbranch_vccz 13f\n\t" \
        "s_and_saveexec_b64 s[66:67], vcc\n\t" \
        "v_mov_b32 %[fet], %[maxs]\n\t" \
        "s_cmp_eq_u32 %[mar], 0\n\t" /* (VolumeView::count_marched: the iterations this lane took) */ \
        "s_cbranch_scc1 131f\n\t" \
        "v_mov_b32 %[fet], v54\n\t" \
        "131:\n\t" \
        VRT_A_FINISH \
        "s_mov_b64 exec, s[66:67]\n\t" \
        "13:\n\t" \
        "v_cmp_ne_u32_e32 vcc, s63, v52\n\t" /* who is live now */ \
        "s_cbranch_vccz 40f\n\t" /* nobody: done */ \
        "v_cndmask_b32_e32 v55, 0, v52, vcc\n\t" /* iterations the lane may take: its clearance (0 for a finished lane) */ \
        "v_min_u32 v55, " VRT_STR(VRT_OWN_CAP) ", v55\n\t" /* ... but no more than a few: the others wait for the longest */ \
        "v_add_u32 v54, v54, v55\n\t" /* it will take them all before the next look */ \
        "20:\n\t" /* ---- iterations for the lanes that have some left (four per trip) ---- */ \
        VRT_A_ITER VRT_A_ITER VRT_A_ITER VRT_A_ITER \
        "s_branch 20b\n\t" \
        "30:\n\t" /* ---- where is every lane now?  request its next byte ---- */ \
        "v_mul_legacy_f32 v48, %[x], %[gx]\n\t" \
        "v_mul_legacy_f32 v49, %[y], %[gy]\n\t" \
        "v_mul_legacy_f32 v50, %[z], %[gz]\n\t" \
        "v_add_f32 v48, v48, %[cx]\n\t" \
        "v_add_f32 v49, v49, %[cy]\n\t" \
        "v_add_f32 v50, v50, %[cz]\n\t" \
        "v_cvt_rpi_i32_f32 v48, v48\n\t" \
        "v_cvt_rpi_i32_f32 v49, v49\n\t" \
        "v_cvt_rpi_i32_f32 v50, v50\n\t" \
        "v_mad_i32_i24 v48, v49, %[pw], v48\n\t" \
        "v_mad_i32_i24 v48, v50, %[pwh], v48\n\t" \
        "v_add_u32 v53, %[idx0], v48\n\t" \
        "global_load_ubyte v52, v53, %[base]\n\t" \
        "s_branch 10b\n\t" \
        "40:\n\t" \
        "s_waitcnt vmcnt(0)\n\t" \
        "s_mov_b64 exec, s[68:69]\n\t" \
        : [x] "+v"(x), [y] "+v"(y), [z] "+v"(z), [dx] "+v"(dx), [dy] "+v"(dy), [dz] "+v"(dz), \
          [gx] "+v"(gx), [gy] "+v"(gy), [gz] "+v"(gz), [cx] "+v"(cx), [cy] "+v"(cy), [cz] "+v"(cz), \
          [idx0] "+v"(idx0), [mat] "+v"(material), [fet] "+v"(fetches) CNT_OPND \
        : [voxoff] "v"(voxoff), [base] "s"(base), [maxs] "s"(maxSteps), [pw] "s"(pw), [pwh] "s"(pwh), [sent] "s"(sentinel), [mar] "s"(marched) \
        : "vcc", "scc", "memory", "v48", "v49", "v50", "v52", "v53", "v54", "v55", \
          "s63", "s64", "s65", "s66", "s67", "s68", "s69")
    if (CNT) { VRT_A_LOOP(VRT_CNT_LOOK, VRT_CNT_FIND, VRT_CNT_OPND); }
    else { VRT_A_LOOP(VRT_CNT_NONE, VRT_CNT_NONE, VRT_CNT_NOOP); }
#undef VRT_A_FINISH
#undef VRT_A_ITER
}

// ---- AO rays from a pool the whole wave draws on ---------------------------------------------------------------------------------
// What an AO trace costs is its ROUNDS: every look-up is a gather the next run depends on, and a wave goes round until its
// neediest lane is done.  The AO rays of a wave point every way and need very different numbers of looks -- on the Mandelbulb 7.8
// on average and 30 for the neediest of 64 (a quarter of the lanes of an AO look-up are live: tools/exp_r4_ao_util.py) -- and the
// long rays belong to the same pixels sample after sample (a pixel in a crevice stays in its crevice): letting a lane go on to
// ITS OWN next ray the moment it is done (first attempt of round 4) measured no gain at all.  So the rays are not the lanes':
// every lane writes the ray of its pixel's next AO sample into a pool in LDS (11 dwords: the state trace_df_fast sets up), and a
// lane that is done takes the NEXT RAY OF THE POOL, whoever's it is -- the slot is the wave's counter + the lane's rank among the
// lanes asking in this round (v_mbcnt: no atomic, the wave runs in lock step) -- and reports what it finds to the owner's counter
// in LDS.  When the pool is empty and a lane rests, the loop returns, the lanes write their next sample's rays and the loop goes
// on where it was: the work of a pixel's four AO rays is spread over the wave, and a wave takes about
// max(all looks / lanes, longest single ray) rounds instead of the sum of four maxima.
// Otherwise df_any_loop: every lane spends its ray's own clearance (at most VRT_OWN_CAP iterations per look), the same fp32
// additions per ray in the same order, the iteration count of a ray its own -- which ray a lane works on changes no result.
// A ray that never enters the volume is handed over with zero deltas and an index whose byte is 0 (the first byte of a field:
// its border): it ends at its first look, as a miss, like any other ray ends.
// LDS of a wave (VRT_AO_SLOT bytes at ldsw): the pool, dword q of the ray in slot k at q * 256 + k * 4 (x y z dx dy dz gx gy gz idx0
// voxoff tag; tag = the column of the ray's pixel | the clearance at its first voxel << 8); at 3072 one counter per COLUMN: rays of
// that pixel that found a solid voxel; at 3328 (CNT) what the count planes report for them.  Column = rank of the pixel's lane
// among the lanes the AO phase runs for; slot = where the ray waits (the owners put the rays that will creep in front).
template <bool CNT>
__device__ __forceinline__ void df_ao_pool_loop(const uint8_t* base, uint32_t maxSteps, int pw, int pwh, uint32_t sentinel,
                                                uint32_t ldsw, uint32_t ldsh, uint32_t count, uint32_t more, uint32_t& next,
                                                float& x, float& y, float& z, float& dx, float& dy, float& dz,
                                                float& gx, float& gy, float& gz, float& cx, float& cy, float& cz,
                                                uint32_t& idx0, uint32_t& voxoff, uint32_t& state, uint32_t& owner,
                                                uint32_t marched, uint32_t& looks)
{
    // vectors of the block: v48..v50 temporaries, v52 the byte read (0xFD: the ray ended in this round, 0xFE: a ray just taken up,
    // 0xFF: the lane rests), v53 its index, v54 = i (iterations of the lane's current ray), v55 = iterations it may take before it
    // looks again, v56 = voxel id on its way, v57 = LDS address of the counter of the ray that id belongs to; scalars: s61 temporary,
    // s62 = 0x80, s63 = 0xFF, s[64:65] lanes with some left, s[66:67] / s[70:71] saved EXEC, s[68:69] EXEC on entry
#define VRT_A_ITER                                               \
        "v_cmp_lt_u32_e32 vcc, 0, v55\n\t"                        \
        "s_cbranch_vccz 30f\n\t"                                  \
        "s_mov_b64 s[64:65], vcc\n\t"                             \
        "s_mov_b64 exec, vcc\n\t"                                 \
        "v_subrev_u32 v55, 1, v55\n\t"                            \
        "v_min3_u32 v48, %[x], %[y], %[z]\n\t"                    \
        "v_cmpx_eq_u32 v48, %[x]\n\t"                             \
        "v_add_f32 %[x], %[x], %[dx]\n\t"                         \
        "s_mov_b64 exec, s[64:65]\n\t"                            \
        "v_cmpx_eq_u32 v48, %[y]\n\t"                             \
        "v_add_f32 %[y], %[y], %[dy]\n\t"                         \
        "s_mov_b64 exec, s[64:65]\n\t"                            \
        "v_cmpx_eq_u32 v48, %[z]\n\t"                             \
        "v_add_f32 %[z], %[z], %[dz]\n\t"                         \
        "s_mov_b64 exec, s[68:69]\n\t"
    // the ids asked for when rays read 0 have arrived: a ray that found a solid voxel counts for its owner (L: a label of its own)
#define VRT_Q_COUNT_ID(L, CNT_SOLID)                             \
        "v_cmp_ne_u32_e32 vcc, 0, v56\n\t"                        \
        "s_cbranch_vccz " L "f\n\t"                               \
        "s_and_saveexec_b64 s[66:67], vcc\n\t"                    \
        "v_mov_b32 v48, 1\n\t"                                    \
        "ds_add_u32 v57, v48\n\t"                                 \
        CNT_SOLID                                                 \
        "s_mov_b64 exec, s[66:67]\n\t"                            \
        L ":\n\t"                                                 \
        "v_mov_b32 v56, 0\n\t"
#define VRT_Q_LOOP(CNT_LOOK, CNT_FIND, CNT_MISS, CNT_SOLID, CNT_OPND) \
    asm volatile( \
        ".p2align 6\n\t" \
        "s_movk_i32 s63, 0xff\n\t" \
        "s_movk_i32 s62, 0x80\n\t" \
        "s_mov_b64 s[68:69], exec\n\t" \
        "v_and_b32 v52, 0xff, %[st]\n\t" /* (between calls: the byte in bits 0..7, the iterations of the lane's ray above) */ \
        "v_lshrrev_b32 v54, 8, %[st]\n\t" \
        "v_mov_b32 v53, %[idx0]\n\t" \
        "v_mov_b32 v56, 0\n\t" \
        "s_branch 125f\n\t" /* (the lanes that rest take their rays first) */ \
        "10:\n\t" /* ---- every lane's byte is here, and the ids asked for in the round before ---- */ \
        CNT_LOOK \
        "s_waitcnt vmcnt(0)\n\t" \
        VRT_Q_COUNT_ID("101", CNT_SOLID) \
        "v_cmp_eq_u32_e32 vcc, 0, v52\n\t" /* solid, border or open cell: the ray ends here; the voxel id says which */ \
        "s_cbranch_vccz 12f\n\t" \
        "s_and_saveexec_b64 s[66:67], vcc\n\t" \
        "v_add_u32 v48, v53, %[voxoff]\n\t" \
        "global_load_ubyte v56, v48, %[base]\n\t" \
        "v_lshl_add_u32 v57, %[own], 2, %[ldsh]\n\t" /* the counter of the pixel this ray belongs to */ \
        CNT_FIND \
        "v_mov_b32 v52, 0xfd\n\t" \
        "s_mov_b64 exec, s[66:67]\n\t" \
        "12:\n\t" \
        "v_cmp_gt_u32_e64 s[64:65], s62, v52\n\t" /* lanes with a clearance (1 .. 127) ... */ \
        "v_sub_u32 v48, %[maxs], v54\n\t" /* ... what is left of their ray's budget ... */ \
        "s_nop 0\n\t" \
        "v_cmp_le_u32_e32 vcc, v48, v52\n\t" /* ... and whether the clearance covers it: a miss at the budget */ \
        "s_and_b64 vcc, vcc, s[64:65]\n\t" \
        "s_cbranch_vccz 125f\n\t" \
        "s_and_saveexec_b64 s[66:67], vcc\n\t" \
        CNT_MISS \
        "v_mov_b32 v52, 0xfd\n\t" \
        "s_mov_b64 exec, s[66:67]\n\t" \
        "125:\n\t" /* ---- lanes whose ray ended in this round, and lanes that rest: the next rays of the pool ---- */ \
        "v_cmp_eq_u32_e32 vcc, 0xfd, v52\n\t" \
        "v_cmp_eq_u32_e64 s[64:65], s63, v52\n\t" \
        "s_nop 1\n\t" \
        "s_or_b64 vcc, vcc, s[64:65]\n\t" \
        "s_cbranch_vccz 13f\n\t" \
        "s_mov_b64 s[70:71], vcc\n\t" \
        "s_and_saveexec_b64 s[66:67], vcc\n\t" \
        "v_mbcnt_lo_u32_b32 v48, s70, 0\n\t" \
        "v_mbcnt_hi_u32_b32 v48, s71, v48\n\t" /* the lane's rank among those asking ... */ \
        "v_add_u32 v48, %[nx], v48\n\t" /* ... + the rays taken so far = its ray's column */ \
        "s_bcnt1_i32_b64 s61, s[70:71]\n\t" \
        "v_cmp_gt_u32_e32 vcc, %[cnt], v48\n\t" /* the pool has that many */ \
        "s_add_u32 %[nx], %[nx], s61\n\t" \
        "s_min_u32 %[nx], %[nx], %[cnt]\n\t" \
        "s_and_saveexec_b64 s[70:71], vcc\n\t" /* EXEC = asking and served; s[70:71] = asking */ \
        "s_cbranch_execz 126f\n\t" \
        "v_lshl_add_u32 v49, v48, 2, %[ldsw]\n\t" \
        "ds_read_b32 v50, v49 offset:2816\n\t" /* the ray's pixel (its counters' column) and the clearance its owner read at its start */ \
        "ds_read_b32 %[x], v49\n\t" \
        "ds_read_b32 %[y], v49 offset:256\n\t" \
        "ds_read_b32 %[z], v49 offset:512\n\t" \
        "ds_read_b32 %[dx], v49 offset:768\n\t" \
        "ds_read_b32 %[dy], v49 offset:1024\n\t" \
        "ds_read_b32 %[dz], v49 offset:1280\n\t" \
        "ds_read_b32 %[gx], v49 offset:1536\n\t" \
        "ds_read_b32 %[gy], v49 offset:1792\n\t" \
        "ds_read_b32 %[gz], v49 offset:2048\n\t" \
        "ds_read_b32 %[idx0], v49 offset:2304\n\t" \
        "ds_read_b32 %[voxoff], v49 offset:2560\n\t" \
        "v_mov_b32 v54, 0\n\t" \
        "s_waitcnt lgkmcnt(0)\n\t" \
        "v_and_b32 %[own], 0xff, v50\n\t" \
        "v_lshrrev_b32 v52, 8, v50\n\t" /* (1 .. maxSteps - 1: the lane goes on to its iterations in this very round) */ \
        "v_mov_b32 v53, %[idx0]\n\t" \
        "v_mul_legacy_f32 %[cx], %[x], %[gx]\n\t" /* c = -(side0 * g): where the ray stands is rint(side * g + c) steps from its start */ \
        "v_mul_legacy_f32 %[cy], %[y], %[gy]\n\t" \
        "v_mul_legacy_f32 %[cz], %[z], %[gz]\n\t" \
        "v_xor_b32 %[cx], 0x80000000, %[cx]\n\t" \
        "v_xor_b32 %[cy], 0x80000000, %[cy]\n\t" \
        "v_xor_b32 %[cz], 0x80000000, %[cz]\n\t" \
        "126:\n\t" \
        "s_andn2_b64 exec, s[70:71], vcc\n\t" /* asking and not served: the lane rests (zero deltas, the 0xFF byte) */ \
        "s_cbranch_execz 127f\n\t" \
        "v_mov_b32 %[dx], 0\n\t" \
        "v_mov_b32 %[dy], 0\n\t" \
        "v_mov_b32 %[dz], 0\n\t" \
        "v_mov_b32 %[gx], 0\n\t" \
        "v_mov_b32 %[gy], 0\n\t" \
        "v_mov_b32 %[gz], 0\n\t" \
        "v_mov_b32 %[cx], 0\n\t" \
        "v_mov_b32 %[cy], 0\n\t" \
        "v_mov_b32 %[cz], 0\n\t" \
        "v_mov_b32 %[idx0], %[sent]\n\t" \
        "v_mov_b32 v53, %[sent]\n\t" \
        "v_mov_b32 v52, s63\n\t" \
        "127:\n\t" \
        "s_mov_b64 exec, s[66:67]\n\t" \
        "s_cmp_lt_u32 %[nx], %[cnt]\n\t" /* the pool is empty, the pixels have more samples, and a lane rests: back to have it refilled */ \
        "s_cbranch_scc1 13f\n\t" \
        "s_cmp_eq_u32 %[more], 0\n\t" \
        "s_cbranch_scc1 13f\n\t" \
        "v_cmp_eq_u32_e32 vcc, s63, v52\n\t" \
        "s_cbranch_vccnz 40f\n\t" \
        "13:\n\t" \
        "v_cmp_ne_u32_e32 vcc, s63, v52\n\t" /* who is live now */ \
        "s_cbranch_vccz 40f\n\t" /* nobody: done, or the pool wants refilling */ \
        "v_cmp_gt_u32_e32 vcc, s62, v52\n\t" /* iterations a lane may take: its clearance (none for a ray just taken up, or a resting lane) */ \
        "v_cndmask_b32_e32 v55, 0, v52, vcc\n\t" \
        "v_min_u32 v55, " VRT_STR(VRT_OWN_CAP) ", v55\n\t" /* ... but no more than a few: the others wait for the longest */ \
        "v_add_u32 v54, v54, v55\n\t" /* it will take them all before the next look */ \
        "20:\n\t" /* ---- iterations for the lanes that have some left (four per trip) ---- */ \
        VRT_A_ITER VRT_A_ITER VRT_A_ITER VRT_A_ITER \
        "s_branch 20b\n\t" \
        "30:\n\t" /* ---- where is every lane now?  request its next byte ---- */ \
        "v_mul_legacy_f32 v48, %[x], %[gx]\n\t" \
        "v_mul_legacy_f32 v49, %[y], %[gy]\n\t" \
        "v_mul_legacy_f32 v50, %[z], %[gz]\n\t" \
        "v_add_f32 v48, v48, %[cx]\n\t" \
        "v_add_f32 v49, v49, %[cy]\n\t" \
        "v_add_f32 v50, v50, %[cz]\n\t" \
        "v_cvt_rpi_i32_f32 v48, v48\n\t" \
        "v_cvt_rpi_i32_f32 v49, v49\n\t" \
        "v_cvt_rpi_i32_f32 v50, v50\n\t" \
        "v_mad_i32_i24 v48, v49, %[pw], v48\n\t" \
        "v_mad_i32_i24 v48, v50, %[pwh], v48\n\t" \
        "v_add_u32 v53, %[idx0], v48\n\t" \
        "global_load_ubyte v52, v53, %[base]\n\t" \
        "s_branch 10b\n\t" \
        "40:\n\t" \
        "s_waitcnt vmcnt(0)\n\t" \
        VRT_Q_COUNT_ID("401", CNT_SOLID) \
        "v_lshl_or_b32 %[st], v54, 8, v52\n\t" \
        "s_waitcnt lgkmcnt(0)\n\t" \
        "s_mov_b64 exec, s[68:69]\n\t" \
        : [x] "+v"(x), [y] "+v"(y), [z] "+v"(z), [dx] "+v"(dx), [dy] "+v"(dy), [dz] "+v"(dz), \
          [gx] "+v"(gx), [gy] "+v"(gy), [gz] "+v"(gz), [cx] "+v"(cx), [cy] "+v"(cy), [cz] "+v"(cz), \
          [idx0] "+v"(idx0), [voxoff] "+v"(voxoff), [st] "+v"(state), [own] "+v"(owner), [nx] "+s"(next) CNT_OPND \
        : [base] "s"(base), [maxs] "s"(maxSteps), [pw] "s"(pw), [pwh] "s"(pwh), [sent] "s"(sentinel), [mar] "s"(marched), \
          [ldsw] "s"(ldsw), [ldsh] "s"(ldsh), [cnt] "s"(count), [more] "s"(more) \
        : "vcc", "scc", "memory", "v48", "v49", "v50", "v52", "v53", "v54", "v55", "v56", "v57", \
          "s61", "s62", "s63", "s64", "s65", "s66", "s67", "s68", "s69", "s70", "s71")
    if (CNT) {
        VRT_Q_LOOP(VRT_CNT_LOOK,
                   "v_add_u32 %[lk], 1, %[lk]\n\t" "ds_add_u32 v57, v54 offset:256\n\t",
                   "v_lshl_add_u32 v49, %[own], 2, %[ldsh]\n\t" "v_mov_b32 v50, %[maxs]\n\t" "s_cmp_eq_u32 %[mar], 0\n\t" "s_cbranch_scc1 141f\n\t" "v_mov_b32 v50, v54\n\t" "141:\n\t" "ds_add_u32 v49, v50 offset:256\n\t",
                   "ds_add_u32 v57, v48 offset:256\n\t",
                   VRT_CNT_OPND);
    } else {
        VRT_Q_LOOP(VRT_CNT_NONE, VRT_CNT_NONE, VRT_CNT_NONE, VRT_CNT_NONE, VRT_CNT_NOOP);
    }
#undef VRT_A_ITER
}

// PF: the look-ups ask for the two neighbouring rows as well (secondary rays: VRT_F_PREFETCH)
// OWN: every lane spends its own clearance (df_any_loop; any-hit rays)
// CNT: the counting twins of the loops (VRT_TRAVERSAL_DF_FAST_CNT): r.fetches = what the march DID for this ray -- the iterations it took
//      (a threshold run's per-axis steps, which is the same number unless two axes tie), or with VolumeView::count_lookups the bytes it
//      asked for (clearance bytes of live lanes, times three where the look-ups prefetch, + the voxel id at the end)
template <class STATS, bool ANYHIT = false, bool PF = false, bool OWN = false, bool CNT = false>
__device__ __forceinline__ void trace_df_fast(const VolumeView& v, f3 start, f3 dir, uint32_t maxSteps, RayInt& r, STATS& stats)
{
    DdaState s;
    dda_entry(v, start, dir, s);
    if (wave_all(oob(v, s.mx, s.my, s.mz))) {
        s.dx = s.dy = s.dz = 0.0f; s.sdx = s.sdy = s.sdz = 0.0f; s.sx = s.sy = s.sz = 0;
        finish(s, 0u, s.mask, 0u, r);
        return;
    }
    dda_rest(dir, s);
    const bool done0 = oob(v, s.mx, s.my, s.mz);
    const uint32_t oct = (uint32_t)(s.sx > 0) | ((uint32_t)(s.sy > 0) << 1) | ((uint32_t)(s.sz > 0) << 2);
    const uint32_t stride = (uint32_t)v.df_stride;
    const int pw = v.W + 2, pwh = pw * (v.H + 2);
    // offsets count from pwh bytes in front of field 0 (room for a prefetch one slice before it: vrt_scene::df_guard, vrt_host.h)
    const uint32_t bias = (uint32_t)pwh, octoff = bias + oct * stride, sentinel = bias + 9u * stride;
    const float kInf = u2f(0x7F800000u);
    // a lane that never enters the volume is finished from the start: zero deltas, the 0xFF byte
    float dx = done0 ? 0.0f : s.dx, dy = done0 ? 0.0f : s.dy, dz = done0 ? 0.0f : s.dz;
    float gx = (!done0 && s.dx < kInf) ? dir.x : 0.0f, gy = (!done0 && s.dy < kInf) ? dir.y : 0.0f, gz = (!done0 && s.dz < kInf) ? dir.z : 0.0f;
    float cx = gx != 0.0f ? -(s.sdx * gx) : 0.0f, cy = gy != 0.0f ? -(s.sdy * gy) : 0.0f, cz = gz != 0.0f ? -(s.sdz * gz) : 0.0f;
    const float gx0 = gx, gy0 = gy, gz0 = gz, cx0 = cx, cy0 = cy, cz0 = cz;     // (CNT: the loops zero a finished lane's copies)
    const uint32_t idx0 = done0 ? sentinel : octoff + (uint32_t)df_index(v, s.mx, s.my, s.mz);
    const uint32_t voxoff = 8u * stride - (octoff - bias);
    uint32_t lmask = s.mask, material = 0u, fetches = 0u, looks = 0u;
    const uint64_t kx = __ballot((s.mask & 1u) != 0u), ky = __ballot((s.mask & 2u) != 0u), kz = __ballot((s.mask & 4u) != 0u);
    float x = s.sdx, y = s.sdy, z = s.sdz;
    // what one step along an axis adds to the index (0 for a lane that never enters the volume)
    const int incx = done0 ? 0 : s.sx, incy = done0 ? 0 : s.sy * pw, incz = done0 ? 0 : s.sz * pwh;
    // the block's scalar operands must BE in scalar registers: values that are uniform but were computed under divergent
    // control flow (secondary rays) may live in vector registers
    const uint64_t b64 = (uint64_t)v.df - (uint64_t)bias;
    const uint8_t* base = (const uint8_t*)(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(b64 >> 32)) << 32) |
                                           (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)b64));      // (the builtin returns int)
    // the loop without a budget (df_prim_loop) for a wave none of whose rays can take maxSteps iterations: a ray
    // steps once per integer plane it crosses, at most tspan * (|dir.x| + |dir.y| + |dir.z|) + 3 times (the margin below covers the
    // rounding of the three factors and the march's own deviation from the ideal line)
    bool thresh = false;
    if (!OWN && __builtin_amdgcn_readfirstlane((int)v.df_thresh) != 0) {      // (primary, bounce and shadow rays; the AO rays' 64 iterations ARE their budget)
        const float bound = s.tspan * ((fabsf(dir.x) + fabsf(dir.y)) + fabsf(dir.z)) * 1.001f + 8.0f;
        thresh = __ballot(!done0 && !(bound < (float)maxSteps)) == 0ull;
    }
    bool prefetching = false;
    if (thresh) {
        df_prim_loop<CNT>(base, __builtin_amdgcn_readfirstlane(pw), __builtin_amdgcn_readfirstlane(pwh), (uint32_t)__builtin_amdgcn_readfirstlane((int)sentinel),
                          x, y, z, dx, dy, dz, gx, gy, gz, cx, cy, cz, idx0, voxoff, lmask, material, kx, ky, kz, incx, incy, incz, looks);
        if (CNT) {
            // the iterations of a march that does not count them: the steps each axis has taken, from the sideDist travelled (the
            // position recovery's own formula); two axes that tie step in ONE iteration of the shader's loop and count twice here
            float qx, qy, qz;
            asm("v_mul_legacy_f32 %0, %1, %2" : "=v"(qx) : "v"(x), "v"(gx0));
            asm("v_mul_legacy_f32 %0, %1, %2" : "=v"(qy) : "v"(y), "v"(gy0));
            asm("v_mul_legacy_f32 %0, %1, %2" : "=v"(qz) : "v"(z), "v"(gz0));
            int nx, ny, nz;
            asm("v_cvt_rpi_i32_f32 %0, %1" : "=v"(nx) : "v"(qx + cx0));
            asm("v_cvt_rpi_i32_f32 %0, %1" : "=v"(ny) : "v"(qy + cy0));
            asm("v_cvt_rpi_i32_f32 %0, %1" : "=v"(nz) : "v"(qz + cz0));
            fetches = (uint32_t)((nx < 0 ? -nx : nx) + (ny < 0 ? -ny : ny) + (nz < 0 ? -nz : nz));
        }
    } else if (ANYHIT && OWN && __builtin_amdgcn_readfirstlane((int)v.df_own) != 0) {
        df_any_loop<CNT>(base, (uint32_t)__builtin_amdgcn_readfirstlane((int)maxSteps), __builtin_amdgcn_readfirstlane(pw), __builtin_amdgcn_readfirstlane(pwh),
                         (uint32_t)__builtin_amdgcn_readfirstlane((int)sentinel), x, y, z, dx, dy, dz, gx, gy, gz, cx, cy, cz, idx0, voxoff, material, fetches,
                         (uint32_t)__builtin_amdgcn_readfirstlane((int)v.count_marched), looks);
    } else {
        const uint32_t pf = PF ? (uint32_t)__builtin_amdgcn_readfirstlane((int)v.df_prefetch) : 0u;
        prefetching = pf != 0u;
        df_fast_loop<CNT>(base, (uint32_t)__builtin_amdgcn_readfirstlane((int)maxSteps), __builtin_amdgcn_readfirstlane(pw), __builtin_amdgcn_readfirstlane(pwh),
                          (uint32_t)__builtin_amdgcn_readfirstlane((int)sentinel), x, y, z, dx, dy, dz, gx, gy, gz, cx, cy, cz, idx0, voxoff, lmask, material, fetches, kx, ky, kz,
                          incx, incy, incz, ANYHIT ? 1u + (uint32_t)__builtin_amdgcn_readfirstlane((int)(v.count_marched != 0u)) : 0u, pf, looks);
    }
    s.sdx = x; s.sdy = y; s.sdz = z;
    uint32_t reported = fetches + (material != 0u ? 1u : 0u);
    if (CNT && v.count_lookups != 0u) {
        // bytes asked for: one clearance byte per look-up of a live lane and the voxel id where a lane read 0 (the loops count both
        // in one register); where the look-ups prefetch the two neighbouring rows, three bytes each (the id then counts thrice too:
        // an upper bound, two bytes per ray above the truth)
        reported = done0 ? 0u : (prefetching ? 3u * looks : looks);
    }
    finish(s, material, lmask, reported, r);
    (void)stats; (void)gx0; (void)gy0; (void)gz0; (void)cx0; (void)cy0; (void)cz0;
}

// ---- AO rays through the wave's pool (df_ao_pool_loop) ---------------------------------------------------------------------------
// trace_df_fast's set-up of one ray (frag:109-144 + the index into its octant's clearance field)
__device__ __forceinline__ void ao_ray_setup(const VolumeView& v, f3 start, f3 dir, AoRay& a)
{
    DdaState s;
    dda_entry(v, start, dir, s);
    dda_rest(dir, s);
    const bool done0 = oob(v, s.mx, s.my, s.mz);
    const uint32_t oct = (uint32_t)(s.sx > 0) | ((uint32_t)(s.sy > 0) << 1) | ((uint32_t)(s.sz > 0) << 2);
    const uint32_t stride = (uint32_t)v.df_stride;
    const int pw = v.W + 2, pwh = pw * (v.H + 2);
    const uint32_t bias = (uint32_t)pwh, octoff = bias + oct * stride;
    const float kInf = u2f(0x7F800000u);
    a.x = s.sdx; a.y = s.sdy; a.z = s.sdz;
    a.dx = done0 ? 0.0f : s.dx; a.dy = done0 ? 0.0f : s.dy; a.dz = done0 ? 0.0f : s.dz;
    a.gx = (!done0 && s.dx < kInf) ? dir.x : 0.0f; a.gy = (!done0 && s.dy < kInf) ? dir.y : 0.0f; a.gz = (!done0 && s.dz < kInf) ? dir.z : 0.0f;
    // a ray that never enters the volume: the first byte of its field -- the border, 0 -- ends it at its first look, as a miss
    a.idx0 = done0 ? octoff : octoff + (uint32_t)df_index(v, s.mx, s.my, s.mz);
    a.voxoff = 8u * stride - (octoff - bias);
}

// a ray into column `col` of the wave's pool (ldsw: the byte address of the wave's LDS); tag: the column of its pixel's counters | the
// clearance its owner read at its first voxel << 8
__device__ __forceinline__ void ao_ray_store(uint32_t ldsw, uint32_t col, const AoRay& a, uint32_t tag)
{
    __attribute__((address_space(3))) uint32_t* p = (__attribute__((address_space(3))) uint32_t*)(ldsw + col * 4u);
    p[0 * 64] = f2u(a.x); p[1 * 64] = f2u(a.y); p[2 * 64] = f2u(a.z);
    p[3 * 64] = f2u(a.dx); p[4 * 64] = f2u(a.dy); p[5 * 64] = f2u(a.dz);
    p[6 * 64] = f2u(a.gx); p[7 * 64] = f2u(a.gy); p[8 * 64] = f2u(a.gz);
    p[9 * 64] = a.idx0; p[10 * 64] = a.voxoff; p[11 * 64] = tag;
}

__device__ __forceinline__ void ao_lane_rest(const VolumeView& v, AoLane& l)
{
    const uint32_t stride = (uint32_t)v.df_stride;
    const int pw = v.W + 2, pwh = pw * (v.H + 2);
    l.x = l.y = l.z = l.dx = l.dy = l.dz = l.gx = l.gy = l.gz = l.cx = l.cy = l.cz = 0.0f;
    l.idx0 = (uint32_t)pwh + 9u * stride; l.voxoff = 0u; l.state = 0xFFu; l.owner = 0u;
}

// One call of the pool loop: `count` rays wait in the pool, `next` of them are taken (in / out), `more`: the pixels have further
// samples, so come back when the pool is empty and a lane rests.  looks (CNT): clearance bytes + ids this LANE asked for.
template <bool CNT>
__device__ __forceinline__ void trace_ao_pool(const VolumeView& v, AoLane& l, uint32_t ldsw, uint32_t count, uint32_t more, uint32_t& next,
                                              uint32_t maxSteps, uint32_t& looks)
{
    const uint32_t stride = (uint32_t)v.df_stride;
    const int pw = v.W + 2, pwh = pw * (v.H + 2);
    const uint32_t bias = (uint32_t)pwh, sentinel = bias + 9u * stride;
    const uint64_t b64 = (uint64_t)v.df - (uint64_t)bias;
    const uint8_t* base = (const uint8_t*)(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(b64 >> 32)) << 32) |
                                           (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)b64));
    const uint32_t lw = (uint32_t)__builtin_amdgcn_readfirstlane((int)ldsw);
    uint32_t nx = (uint32_t)__builtin_amdgcn_readfirstlane((int)next);
    df_ao_pool_loop<CNT>(base, (uint32_t)__builtin_amdgcn_readfirstlane((int)maxSteps), __builtin_amdgcn_readfirstlane(pw), __builtin_amdgcn_readfirstlane(pwh),
                         (uint32_t)__builtin_amdgcn_readfirstlane((int)sentinel), lw, lw + 3072u, (uint32_t)__builtin_amdgcn_readfirstlane((int)count),
                         (uint32_t)__builtin_amdgcn_readfirstlane((int)more), nx,
                         l.x, l.y, l.z, l.dx, l.dy, l.dz, l.gx, l.gy, l.gz, l.cx, l.cy, l.cz, l.idx0, l.voxoff, l.state, l.owner,
                         (uint32_t)__builtin_amdgcn_readfirstlane((int)v.count_marched), looks);
    next = nx;
}
#endif

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- HOST STUBS of this header's device-only functions -----------------------------------------------------------
// host pass of a .hip file / the host build of the unit tests: parsed, never run (the loop is gfx950 assembly)
template <class STATS, bool ANYHIT = false, bool PF = false, bool OWN = false, bool CNT = false>
VRT_HD void trace_df_fast(const VolumeView&, f3, f3, uint32_t, RayInt&, STATS&) {}
VRT_HD void ao_ray_setup(const VolumeView&, f3, f3, AoRay&) {}
VRT_HD void ao_ray_store(uint32_t, uint32_t, const AoRay&, uint32_t) {}
VRT_HD void ao_lane_rest(const VolumeView&, AoLane&) {}
template <bool CNT> VRT_HD void trace_ao_pool(const VolumeView&, AoLane&, uint32_t, uint32_t, uint32_t, uint32_t&, uint32_t, uint32_t&) {}
#endif

} // namespace vrt
