// vrt_dda.h -- the DDA every march is made of, host + device: boxIntersection and the set-up of voxel_volume.frag:109-144
// (DdaState, dda_entry / dda_rest / dda_setup), one literal iteration (VRT_DDA_STEP), the iterations that only advance
// sideDist (dda_advance; on the device also the forms for wave-uniform control flow, which narrow EXEC themselves), the
// recovery of mapPos from the sideDist travelled (steps_signed) and the wave votes (wave_min_vote: how far may the wave run).
// The device-only functions have no host form: host code reaches them nowhere.
#pragma once

#include "vrt_volume.h"

namespace vrt {

// ---- boxIntersection + DDA setup (frag:109-144) -------------------------------------------------------

struct DdaState {
    f3 p;                     // boxIntersection() result
    int mx, my, mz;           // mapPos
    float sdx, sdy, sdz;      // sideDist
    float dx, dy, dz;         // deltaDist
    int sx, sy, sz;           // rayStep
    uint32_t mask;            // rule A initial mask
    float ivx, ivy, ivz;      // 1 / dir (dda_entry -> dda_rest)
    float tspan;              // length of the ray inside the box, from where the march starts to where it leaves (0: never inside)
};

// float -> int as the device converts (v_cvt_i32_f32: saturating, NaN -> 0), spelled out for the host build, where a value
// outside the int range is undefined behaviour: a far origin, or a direction 2^60 long (the +0.1 of boxIntersection is in units of
// it), puts boxIntersection's point there
VRT_HD int to_int_sat(float x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (int)x;
#else
    return x != x ? 0 : x >= 2147483648.0f ? 2147483647 : x <= -2147483648.0f ? (-2147483647 - 1) : (int)x;
#endif
}

// boxIntersection (frag:109-125) and the first mapPos (frag:135): everything needed to know whether the march can
// leave the volume in iteration 0.
VRT_HD void dda_entry(const VolumeView& v, f3 start, f3 dir, DdaState& s)
{
    float ivx = 1.0f / dir.x, ivy = 1.0f / dir.y, ivz = 1.0f / dir.z;
    float t1x = (-start.x) * ivx, t2x = ((float)v.W - start.x) * ivx;
    float t1y = (-start.y) * ivy, t2y = ((float)v.H - start.y) * ivy;
    float t1z = (-start.z) * ivz, t2z = ((float)v.D - start.z) * ivz;
    float tnx = fminf(t1x, t2x), tny = fminf(t1y, t2y), tnz = fminf(t1z, t2z);
    float txx = fmaxf(t1x, t2x), txy = fmaxf(t1y, t2y), txz = fmaxf(t1z, t2z);
    float tmin = fmaxf(tnx, fmaxf(tny, tnz));
    float tmax = fminf(txx, fminf(txy, txz));
    s.p = start;
    s.mask = 0;
    if (tmin >= 0.0f && tmax >= tmin) {
        float t = tmin + 0.1f;
        s.p = mk3(start.x + t * dir.x, start.y + t * dir.y, start.z + t * dir.z);
        s.mask = (uint32_t)(tnx == tmin) | ((uint32_t)(tny == tmin) << 1) | ((uint32_t)(tnz == tmin) << 2);
    }
    s.mx = to_int_sat(floorf(s.p.x)); s.my = to_int_sat(floorf(s.p.y)); s.mz = to_int_sat(floorf(s.p.z));
    s.ivx = ivx; s.ivy = ivy; s.ivz = ivz;
    const float t0 = fmaxf(tmin, 0.0f);
    s.tspan = tmax >= t0 ? tmax - t0 : 0.0f;
}

// deltaDist, rayStep, sideDist (frag:136-144)
VRT_HD void dda_rest(f3 dir, DdaState& s)
{
    s.dx = fabsf(s.ivx); s.dy = fabsf(s.ivy); s.dz = fabsf(s.ivz);
    float gx = fsign(dir.x), gy = fsign(dir.y), gz = fsign(dir.z);
    s.sx = (int)gx; s.sy = (int)gy; s.sz = (int)gz;
    s.sdx = ((gx * ((float)s.mx - s.p.x) + gx * 0.5f) + 0.5f) * s.dx;
    s.sdy = ((gy * ((float)s.my - s.p.y) + gy * 0.5f) + 0.5f) * s.dy;
    s.sdz = ((gz * ((float)s.mz - s.p.z) + gz * 0.5f) + 0.5f) * s.dz;
}

VRT_HD void dda_setup(const VolumeView& v, f3 start, f3 dir, DdaState& s)
{
    dda_entry(v, start, dir, s);
    dda_rest(dir, s);
}

// One literal DDA iteration's advance (frag:164-170).  sideDist is never negative, so the order of the
// floats is the order of their bit patterns: mask_a = (side_a <= min(side_b, side_c)) == (bits_a == min3(bits)).
// (Integer min/compare need no NaN canonicalisation, which halves the instruction count of this block.)
#define VRT_DDA_STEP(S, MASK)                                                         \
    do {                                                                              \
        uint32_t bx_ = f2u((S).sdx), by_ = f2u((S).sdy), bz_ = f2u((S).sdz);          \
        uint32_t mn_ = umin3(bx_, by_, bz_);                                          \
        bool m0_ = bx_ == mn_, m1_ = by_ == mn_, m2_ = bz_ == mn_;                    \
        (MASK) = (uint32_t)m0_ | ((uint32_t)m1_ << 1) | ((uint32_t)m2_ << 2);         \
        (S).sdx = m0_ ? (S).sdx + (S).dx : (S).sdx; (S).mx += m0_ ? (S).sx : 0;       \
        (S).sdy = m1_ ? (S).sdy + (S).dy : (S).sdy; (S).my += m1_ ? (S).sy : 0;       \
        (S).sdz = m2_ ? (S).sdz + (S).dz : (S).sdz; (S).mz += m2_ ? (S).sz : 0;       \
    } while (0)

VRT_HD void finish(const DdaState& s, uint32_t material, uint32_t mask, uint32_t fetches, RayInt& r)
{
    r.pos = s.p; r.side = mk3(s.sdx, s.sdy, s.sdz); r.delta = mk3(s.dx, s.dy, s.dz);
    r.sx = s.sx; r.sy = s.sy; r.sz = s.sz; r.mx = s.mx; r.my = s.my; r.mz = s.mz;
    r.material = material; r.mask = mask; r.fetches = fetches; r.dbg0 = 0; r.dbg1 = 0;
}

// rint(x) as an int; saturating, NaN -> 0 (what v_cvt_i32_f32 does; spelled out for the host build: to_int_sat)
VRT_HD int steps_taken(float x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (int)rintf(x);
#else
    return to_int_sat(rintf(x));
#endif
}

// Signed number of steps an axis took while its sideDist grew by dside: floor(dside * g + 1/2), g = +-1/delta (or 0 for
// an axis that cannot step: its sideDist is +inf, inf - inf = NaN, and the DX9-rule multiply makes NaN * 0 = 0).
// Two VALU ops: v_mul_legacy_f32 + v_cvt_rpi_i32_f32 (round to nearest by floor(x + 0.5) in one instruction).
VRT_HD int steps_signed(float dside, float g)
{
#if defined(__HIP_DEVICE_COMPILE__)
    int n;
    float q;
    asm("v_mul_legacy_f32 %0, %1, %2" : "=v"(q) : "v"(dside), "v"(g));
    asm("v_cvt_rpi_i32_f32 %0, %1" : "=v"(n) : "v"(q));
    return n;
#else
    return g == 0.0f ? 0 : to_int_sat(floorf(dside * g + 0.5f));
#endif
}

// One DDA iteration that only advances sideDist (frag:164-170 without the mapPos / mask bookkeeping).
// Device: 7 VALU ops -- one three-way integer min, then per axis a v_cmpx that narrows EXEC to the lanes whose axis holds the
// minimum and a v_add_f32 that runs under it (the compiler's form is compare + select + add = 10).  EXEC is put back
// from a scalar copy after each axis; the scalar moves issue beside other waves' vector work.
VRT_HD void dda_advance(DdaState& s)
{
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t mn;
    uint64_t saved;
    asm volatile("v_min3_u32 %[mn], %[x], %[y], %[z]\n\t"
                 "s_mov_b64 %[sv], exec\n\t"
                 "v_cmpx_eq_u32 %[mn], %[x]\n\t"
                 "v_add_f32 %[x], %[x], %[dx]\n\t"
                 "s_mov_b64 exec, %[sv]\n\t"
                 "v_cmpx_eq_u32 %[mn], %[y]\n\t"
                 "v_add_f32 %[y], %[y], %[dy]\n\t"
                 "s_mov_b64 exec, %[sv]\n\t"
                 "v_cmpx_eq_u32 %[mn], %[z]\n\t"
                 "v_add_f32 %[z], %[z], %[dz]\n\t"
                 "s_mov_b64 exec, %[sv]"
                 : [x] "+v"(s.sdx), [y] "+v"(s.sdy), [z] "+v"(s.sdz), [mn] "=&v"(mn), [sv] "=&s"(saved)
                 : [dx] "v"(s.dx), [dy] "v"(s.dy), [dz] "v"(s.dz)
                 : "vcc");
#else
    uint32_t bx = f2u(s.sdx), by = f2u(s.sdy), bz = f2u(s.sdz);
    uint32_t mn = umin3(bx, by, bz);
    s.sdx = bx == mn ? s.sdx + s.dx : s.sdx;
    s.sdy = by == mn ? s.sdy + s.dy : s.sdy;
    s.sdz = bz == mn ? s.sdz + s.dz : s.sdz;
#endif
}

#if defined(__HIP_DEVICE_COMPILE__)
// The same iteration for use in wave-uniform control flow: only the lanes of `live` advance (EXEC is narrowed to
// live & "this axis holds the minimum" per axis and put back to its value on entry at the end).
__device__ __forceinline__ void dda_advance_live(DdaState& s, uint64_t live)
{
    uint32_t mn;
    uint64_t entry;
    asm volatile("v_min3_u32 %[mn], %[x], %[y], %[z]\n\t"
                 "s_mov_b64 %[en], exec\n\t"
                 "s_mov_b64 exec, %[lv]\n\t"
                 "v_cmpx_eq_u32 %[mn], %[x]\n\t"
                 "v_add_f32 %[x], %[x], %[dx]\n\t"
                 "s_mov_b64 exec, %[lv]\n\t"
                 "v_cmpx_eq_u32 %[mn], %[y]\n\t"
                 "v_add_f32 %[y], %[y], %[dy]\n\t"
                 "s_mov_b64 exec, %[lv]\n\t"
                 "v_cmpx_eq_u32 %[mn], %[z]\n\t"
                 "v_add_f32 %[z], %[z], %[dz]\n\t"
                 "s_mov_b64 exec, %[en]"
                 : [x] "+v"(s.sdx), [y] "+v"(s.sdy), [z] "+v"(s.sdz), [mn] "=&v"(mn), [en] "=&s"(entry)
                 : [dx] "v"(s.dx), [dy] "v"(s.dy), [dz] "v"(s.dz), [lv] "s"(live)
                 : "vcc");
}
// ... and handing out the EXEC mask each v_cmpx leaves behind: it IS that axis' mask bit for the live lanes.
__device__ __forceinline__ void dda_advance_live_masks(DdaState& s, uint64_t live, uint64_t& kx, uint64_t& ky, uint64_t& kz)
{
    uint32_t mn;
    uint64_t entry;
    asm volatile("v_min3_u32 %[mn], %[x], %[y], %[z]\n\t"
                 "s_mov_b64 %[en], exec\n\t"
                 "s_mov_b64 exec, %[lv]\n\t"
                 "v_cmpx_eq_u32 %[mn], %[x]\n\t"
                 "s_mov_b64 %[kx], exec\n\t"
                 "v_add_f32 %[x], %[x], %[dx]\n\t"
                 "s_mov_b64 exec, %[lv]\n\t"
                 "v_cmpx_eq_u32 %[mn], %[y]\n\t"
                 "s_mov_b64 %[ky], exec\n\t"
                 "v_add_f32 %[y], %[y], %[dy]\n\t"
                 "s_mov_b64 exec, %[lv]\n\t"
                 "v_cmpx_eq_u32 %[mn], %[z]\n\t"
                 "s_mov_b64 %[kz], exec\n\t"
                 "v_add_f32 %[z], %[z], %[dz]\n\t"
                 "s_mov_b64 exec, %[en]"
                 : [x] "+v"(s.sdx), [y] "+v"(s.sdy), [z] "+v"(s.sdz), [mn] "=&v"(mn), [en] "=&s"(entry),
                   [kx] "=&s"(kx), [ky] "=&s"(ky), [kz] "=&s"(kz)
                 : [dx] "v"(s.dx), [dy] "v"(s.dy), [dz] "v"(s.dz), [lv] "s"(live)
                 : "vcc");
}
// A whole run of kw >= 1 iterations for the lanes of `live` in one block: kw - 1 iterations whose masks nobody reads, then
// one that hands out its three EXEC masks.  EXEC is saved and put back once per run instead of once per iteration, and the
// counter lives in the block: 5 scalar instructions per iteration (three EXEC reloads, decrement, branch) instead of 8.
// The scalar unit matters: the kernel issues almost as many scalar as vector instructions.
__device__ __forceinline__ void dda_run_live_masks(DdaState& s, uint64_t live, uint32_t kw, uint64_t& kx, uint64_t& ky, uint64_t& kz,
                                                   float& ox, float& oy, float& oz)
{
    uint32_t mn, cnt;
    uint64_t entry;
#define VRT_DDA_ITER                                           \
                 "s_mov_b64 exec, %[lv]\n\t"                    \
                 "v_min3_u32 %[mn], %[x], %[y], %[z]\n\t"       \
                 "v_cmpx_eq_u32 %[mn], %[x]\n\t"                \
                 "v_add_f32 %[x], %[x], %[dx]\n\t"              \
                 "s_mov_b64 exec, %[lv]\n\t"                    \
                 "v_cmpx_eq_u32 %[mn], %[y]\n\t"                \
                 "v_add_f32 %[y], %[y], %[dy]\n\t"              \
                 "s_mov_b64 exec, %[lv]\n\t"                    \
                 "v_cmpx_eq_u32 %[mn], %[z]\n\t"                \
                 "v_add_f32 %[z], %[z], %[dz]\n\t"
    // half of all runs are a single iteration: they take the first branch and nothing else; longer runs do their plain
    // iterations four per loop trip (a taken branch stalls the wave's instruction stream), the odd one, two or three first
    // (the block also keeps sideDist as it was on entry, ox/oy/oz: the compiler's own copies around an in/out operand are
    // three before and two after)
    asm volatile("s_mov_b64 %[en], exec\n\t"
                 "v_mov_b32 %[ox], %[x]\n\t"
                 "v_mov_b32 %[oy], %[y]\n\t"
                 "v_mov_b32 %[oz], %[z]\n\t"
                 "s_cmp_eq_u32 %[kw], 1\n\t"
                 "s_cbranch_scc1 2f\n\t"
                 "s_sub_u32 %[cnt], %[kw], 1\n\t"            // plain iterations, >= 1
                 "s_bitcmp0_b32 %[cnt], 0\n\t"
                 "s_cbranch_scc1 3f\n\t"
                 VRT_DDA_ITER
                 "3:\n\t"
                 "s_bitcmp0_b32 %[cnt], 1\n\t"
                 "s_cbranch_scc1 4f\n\t"
                 VRT_DDA_ITER
                 VRT_DDA_ITER
                 "4:\n\t"
                 "s_lshr_b32 %[cnt], %[cnt], 2\n\t"          // quads; SCC = (quads != 0)
                 "s_cbranch_scc0 2f\n\t"
                 "s_sub_u32 %[cnt], %[cnt], 1\n\t"
                 "1:\n\t"
                 VRT_DDA_ITER
                 VRT_DDA_ITER
                 VRT_DDA_ITER
                 VRT_DDA_ITER
                 "s_sub_u32 %[cnt], %[cnt], 1\n\t"
                 "s_cbranch_scc0 1b\n\t"
                 "2:\n\t"
                 "s_mov_b64 exec, %[lv]\n\t"
                 "v_min3_u32 %[mn], %[x], %[y], %[z]\n\t"
                 "v_cmpx_eq_u32 %[mn], %[x]\n\t"
                 "s_mov_b64 %[kx], exec\n\t"
                 "v_add_f32 %[x], %[x], %[dx]\n\t"
                 "s_mov_b64 exec, %[lv]\n\t"
                 "v_cmpx_eq_u32 %[mn], %[y]\n\t"
                 "s_mov_b64 %[ky], exec\n\t"
                 "v_add_f32 %[y], %[y], %[dy]\n\t"
                 "s_mov_b64 exec, %[lv]\n\t"
                 "v_cmpx_eq_u32 %[mn], %[z]\n\t"
                 "s_mov_b64 %[kz], exec\n\t"
                 "v_add_f32 %[z], %[z], %[dz]\n\t"
                 "s_mov_b64 exec, %[en]"
                 : [x] "+v"(s.sdx), [y] "+v"(s.sdy), [z] "+v"(s.sdz), [mn] "=&v"(mn), [en] "=&s"(entry), [cnt] "=&s"(cnt),
                   [kx] "=&s"(kx), [ky] "=&s"(ky), [kz] "=&s"(kz), [ox] "=&v"(ox), [oy] "=&v"(oy), [oz] "=&v"(oz)
                 : [dx] "v"(s.dx), [dy] "v"(s.dy), [dz] "v"(s.dz), [lv] "s"(live), [kw] "s"(kw)
                 : "vcc", "scc");
#undef VRT_DDA_ITER
}
#endif

#if defined(__HIP_DEVICE_COMPILE__)
// this lane's bits of three wave-uniform lane masks as 1 | 2 | 4: v_cndmask with the mask as its condition operand
__device__ __forceinline__ uint32_t lane_bits(uint64_t kx, uint64_t ky, uint64_t kz)
{
    uint32_t bx, by, bz;
    asm("v_cndmask_b32_e64 %0, 0, 1, %1" : "=v"(bx) : "s"(kx));
    asm("v_cndmask_b32_e64 %0, 0, 2, %1" : "=v"(by) : "s"(ky));
    asm("v_cndmask_b32_e64 %0, 0, 4, %1" : "=v"(bz) : "s"(kz));
    return bx | by | bz;
}
#endif

// ---- wavefront votes (device: the 64 lanes of a gfx950 wave; host tests: a single lane) ------------------

VRT_HD bool wave_all(bool p)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __all(p) != 0;
#else
    return p;
#endif
}
VRT_HD bool wave_any(bool p)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __any(p) != 0;
#else
    return p;
#endif
}
// min over the active lanes of k (k <= 63), by binary search over ballots: 6 votes, no cross-lane data movement.
VRT_HD uint32_t wave_min_u6(uint32_t k)
{
#if defined(__HIP_DEVICE_COMPILE__)
    if (__ballot(true) == ~0ull) {
        // all 64 lanes live (the common case): DPP min-scan, total in lane 63.  row_shr:1,2,4,8 fold each row of 16,
        // row_bcast:15 / :31 fold the rows; lanes without a source keep `old` = 63, the identity.
        // v_min_u32 with the DPP modifier on its first source: one VALU op per stage (the builtin form costs three:
        // mov, mov_dpp, min).  A lane whose DPP source does not exist is disabled for that op and keeps its value.
        // s_nop 1 = the two wait states gfx9 needs between a VALU write of a VGPR and a DPP read of it.
        uint32_t v = k, total;
        asm volatile("s_nop 1\n\t"
                     "v_min_u32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
                     "s_nop 1\n\t"
                     "v_min_u32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n\t"
                     "s_nop 1\n\t"
                     "v_min_u32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"
                     "s_nop 1\n\t"
                     "v_min_u32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf\n\t"
                     "s_nop 1\n\t"
                     "v_min_u32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
                     "s_nop 1\n\t"
                     "v_min_u32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
                     "s_nop 1\n\t"
                     "v_readlane_b32 %1, %0, 63\n\t"
                     "s_nop 3"
                     : "+v"(v), "=s"(total));
        return total;
    }
    uint32_t m = 0;                                           // partial waves: binary search over ballots
#pragma unroll
    for (uint32_t bit = 32u; bit != 0u; bit >>= 1)
        if (__ballot(k < (m | bit)) == 0ull) m |= bit;
    return m;
#else
    return k;
#endif
}

// One vote for "is every lane finished" and "how far may the wave run": finished lanes vote VRT_VOTE_DONE, live lanes
// their clearance (1..63); the minimum is VRT_VOTE_DONE exactly when nobody is live.
#define VRT_VOTE_DONE 0xFFFFu
VRT_HD uint32_t wave_min_vote(uint32_t k)
{
#if defined(__HIP_DEVICE_COMPILE__)
    // Half of all look-ups end with a clearance of 1 somewhere in the wave, another quarter with 2 or 3: one compare
    // each answers those before the 7-op reduction is needed (votes are >= 1; VRT_VOTE_DONE matches none of them).
    if (__ballot(k == 1u) != 0ull) return 1u;
    const bool full = __ballot(true) == ~0ull;
    if (!full) {                                               // secondary rays of a partly hit wave: the reduction below is
        if (__ballot(k == 2u) != 0ull) return 2u;              // the 6-vote binary search, worth two more shortcuts
        if (__ballot(k == 3u) != 0ull) return 3u;
    }
    if (full) {
        uint32_t v = k, total;
        asm volatile("s_nop 1\n\t"
                     "v_min_u32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
                     "s_nop 1\n\t"
                     "v_min_u32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n\t"
                     "s_nop 1\n\t"
                     "v_min_u32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"
                     "s_nop 1\n\t"
                     "v_min_u32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf\n\t"
                     "s_nop 1\n\t"
                     "v_min_u32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
                     "s_nop 1\n\t"
                     "v_min_u32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
                     "s_nop 1\n\t"
                     "v_readlane_b32 %1, %0, 63\n\t"
                     "s_nop 3"
                     : "+v"(v), "=s"(total));
        return total;
    }
    if (__ballot(k != VRT_VOTE_DONE) == 0ull) return VRT_VOTE_DONE;
    return wave_min_u6(k < 63u ? k : 63u);
#else
    return k;
#endif
}

} // namespace vrt
