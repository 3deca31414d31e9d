// vrt_march_brick.h -- BRICK: the DF march over the two-level clearance of a brick scene (brick_clear, trace_brick with
// its threshold runs brick_march_thresh) and its AO forms (trace_brick_own, the pool: BrickAoLane, brick_ao_*).
// Included by vrt_traverse.h.  Plain C++ except axis_run, one block of gfx950 assembly (device pass only); trace_brick also
// runs on the host in the unit tests, the device-only functions have empty host stubs at the end.
#pragma once

#include "vrt_dda.h"     // (over vrt_volume.h: the data types and the DDA)

namespace vrt {

#ifndef VRT_THRESH_SPREAD
#define VRT_THRESH_SPREAD 1          // brick_march_thresh: a lane's threshold run uses at most this many times the wave's smallest clearance (measured on config 5: 1 -> 3.38 ms, 2 -> 3.46, 4 -> 3.48, no cap -> 13 ms: the others wait for the lane that goes furthest)
#endif
#ifndef VRT_OWN_CAP_BRICK
#define VRT_OWN_CAP_BRICK 8          // ... in the brick march, whose look-ups cost more (trace_brick_own: 5.07 ms at 4, 5.00 at 8)
#endif

// ---- BRICK: the DF march over a sparse volume -------------------------------------------------------------------------
// Same loop as DF -- the wave agrees on a number of iterations nobody needs a memory test for, runs them with the shader's
// own fp32 additions, looks again -- with the clearance read from two levels: in an EMPTY brick one byte per brick and
// octant says how many bricks are clear (the voxel's own clearance follows from where it sits in its brick), in an OCCUPIED
// brick one byte per voxel and octant (looking through the neighbouring bricks, up to 16 voxels).  Any lower bound of the
// true clearance gives the same hit (a run only ever skips voxels that are certainly empty), so the result is the dense
// DF's and the oracle's bit for bit; empty space costs one byte per BRICK in memory and traffic.

// One look-up of the brick march: the clearance at voxel (mx, my, mz) for a ray of octant `oct` (sx, sy, sz its steps), and the
// voxel's id where that is 0 inside an occupied brick.  One 8-byte load answers for an empty brick, the border and an open
// brick; only a lane inside an OCCUPIED brick goes on to its per-voxel byte.  The arithmetic for the empty-brick answer runs
// for every lane (a dozen instructions, no branch); 32-bit offsets while the padded grid is below 2^29 bricks.
#if defined(VRT_TRACE_COUNTERS) && defined(__HIPCC__)
// development build only: look-ups of the brick march by kind, summed over the lanes of all rays (vrt_debug_counters).
// Defined in one object: part 0 of vrt_device.hip, which holds the brick march's kernels and debug_brick_counts.  Every other
// object that includes this header counts into a copy of its own that nobody reads (the brick march's counting twins of part 2).
#if !(defined(VRT_K1_PART) && VRT_K1_PART == 0)
static
#endif
__device__ unsigned long long g_vrt_brick_counts[4];   // lanes looking up, ... in an occupied brick, ... that found a solid voxel, ... in the border / an open brick
#endif
VRT_HD uint32_t brick_clear(const VolumeView& v, int mx, int my, int mz, uint32_t oct, int sx, int sy, int sz, uint32_t& material, uint32_t* bytes = nullptr)
{
    const uint32_t bx = (uint32_t)((mx >> 3) + 1), by = (uint32_t)((my >> 3) + 1), bz = (uint32_t)((mz >> 3) + 1);   // (-1 >> 3 = -1: the border brick)
    const uint32_t bi = bx + (uint32_t)mul24((int)by, v.pbx) + (uint32_t)mul24((int)bz, v.pbx * v.pby);
    const uint64_t e = v.bentry[bi];
    const uint32_t lo = (uint32_t)e, c = ((uint32_t)(e >> 32) >> (oct * 4u)) & 15u, ptr = lo & 0xFFFFFFu;
    const uint32_t lx = (uint32_t)mx & 7u, ly = (uint32_t)my & 7u, lz = (uint32_t)mz & 7u;
    // an empty brick with c - 1 empty bricks behind it on every axis: the room to the brick's far face is (l ^ 7) + 1 looking
    // up an axis, l + 1 looking down
    const uint32_t rx = (lx ^ (sx > 0 ? 7u : 0u)) + 1u, ry = (ly ^ (sy > 0 ? 7u : 0u)) + 1u, rz = (lz ^ (sz > 0 ? 7u : 0u)) + 1u;
    uint32_t k = (c - 1u) * 8u + umin3(rx, ry, rz);
    k = k < 127u ? k : 127u;
    const bool open = v.brick_open != 0u && ((lo >> (24u + oct)) & 1u) != 0u;     // an open brick: the march ends here as a miss
    uint32_t clear = (c != 0u && !open) ? k : 0u;                                  // (c == 0 and no pool brick: the border -- the ray has left)
    if (c == 0u && ptr - 1u < 0xFFFFFEu) {
        const uint32_t l = lx | (ly << 3) | (lz << 6);
        clear = v.bfine[(size_t)(ptr - 1u) * 4096u + (size_t)(oct * 512u + l)];
        if (clear == 0u) material = v.bpool[(size_t)(ptr - 1u) * 512u + (size_t)l];
        if (bytes) *bytes += clear == 0u ? 2u : 1u;
    }
    if (bytes) *bytes += 8u;
#if defined(VRT_TRACE_COUNTERS) && defined(__HIP_DEVICE_COMPILE__)
    {
        const bool occb = c == 0u && ptr - 1u < 0xFFFFFEu;
        const unsigned long long n0 = __builtin_popcountll(__ballot(true)), n1 = __builtin_popcountll(__ballot(occb)),
                                 n2 = __builtin_popcountll(__ballot(occb && clear == 0u)), n3 = __builtin_popcountll(__ballot(!occb && clear == 0u));
        if (__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) == 0u || __ballot(true) != ~0ull) {
            // one lane of the active set adds for all (the first active lane)
            const unsigned long long act = __ballot(true);
            if ((threadIdx.x & 63u) == (unsigned)__builtin_ctzll(act)) {
                atomicAdd(&g_vrt_brick_counts[0], n0); atomicAdd(&g_vrt_brick_counts[1], n1);
                atomicAdd(&g_vrt_brick_counts[2], n2); atomicAdd(&g_vrt_brick_counts[3], n3);
            }
        }
    }
#endif
    return clear;
}

#if defined(__HIP_DEVICE_COMPILE__)
// One axis of a threshold run under the EXEC mask it is entered with: x (+)= dx while x <= T, at most 128 times (v_cmpx narrows
// EXEC monotonically -- a lane that has passed T stays out -- so nothing is put back between steps; four steps per trip)
__device__ __forceinline__ void axis_run(float& x, float dx, float T)
{
    uint64_t saved;
    uint32_t cnt;
    asm volatile("s_mov_b64 %[sv], exec\n\t"
                 "s_movk_i32 %[cnt], 31\n\t"
                 "1:\n\t"
                 "v_cmpx_ge_f32 %[T], %[x]\n\t"
                 "v_add_f32 %[x], %[x], %[dx]\n\t"
                 "v_cmpx_ge_f32 %[T], %[x]\n\t"
                 "v_add_f32 %[x], %[x], %[dx]\n\t"
                 "v_cmpx_ge_f32 %[T], %[x]\n\t"
                 "v_add_f32 %[x], %[x], %[dx]\n\t"
                 "v_cmpx_ge_f32 %[T], %[x]\n\t"
                 "v_add_f32 %[x], %[x], %[dx]\n\t"
                 "s_cbranch_execz 2f\n\t"
                 "s_sub_u32 %[cnt], %[cnt], 1\n\t"
                 "s_cbranch_scc0 1b\n\t"
                 "2:\n\t"
                 "s_mov_b64 exec, %[sv]"
                 : [x] "+v"(x), [sv] "=&s"(saved), [cnt] "=&s"(cnt)
                 : [dx] "v"(dx), [T] "v"(T)
                 : "vcc", "scc");
}

// The brick march without a budget, its long runs by threshold (df_prim_loop's scheme in the generic loop): a run of up to four
// iterations for everybody when some lane's clearance is that small (they leave the mask bits behind that a hit needs), else
// every lane steps each axis on its own while its sideDist is <= the lane's threshold min(side + (c - 1) delta) (1 - 2^-16) --
// one compare and one addition per step, every lane its own clearance.  Entered only by waves none of whose rays can take
// maxSteps iterations (trace_brick); primary, bounce and shadow rays.
template <class STATS, bool CNT = false>
__device__ __forceinline__ void brick_march_thresh(const VolumeView& v, DdaState& s, f3 dir, RayInt& r, STATS& stats)
{
    asm volatile("" : "+v"(s.dx), "+v"(s.dy), "+v"(s.dz));
    uint64_t kx = __ballot((s.mask & 1u) != 0u), ky = __ballot((s.mask & 2u) != 0u), kz = __ballot((s.mask & 4u) != 0u);
    uint32_t lmask = s.mask, material = 0u, clear = 63u;
    // (CNT, VRT_TRAVERSAL_BRICK_CNT: the steps the axes take, which is the iteration count unless two of them tie, and the bytes the
    // look-ups ask for; the product kernels are the CNT = false instantiations)
    constexpr bool cnt = CNT;
    uint32_t steps = 0u, bytes = 0u;
    bool done = oob(v, s.mx, s.my, s.mz);
    const uint32_t oct = (uint32_t)(s.sx > 0) | ((uint32_t)(s.sy > 0) << 1) | ((uint32_t)(s.sz > 0) << 2);
    const float kInf = u2f(0x7F800000u);
    const float gx = s.dx < kInf ? dir.x : 0.0f, gy = s.dy < kInf ? dir.y : 0.0f, gz = s.dz < kInf ? dir.z : 0.0f;
    // (every look-up is followed by at least one step of every live lane: the count only ends a wave whose rays cannot step --
    // direction (0, 0, 0): the shader's loop spins to its budget and misses, and so does a lane still live here)
    for (uint32_t guard = 0; guard < 16384u; guard++) {
        if (!done) {
            uint32_t m = 0u;
            clear = brick_clear(v, s.mx, s.my, s.mz, oct, s.sx, s.sy, s.sz, m, cnt ? &bytes : nullptr);
            st_lookup(stats);
            if (clear == 0u) {                                 // solid, the border, or an open brick
                if (!oob(v, s.mx, s.my, s.mz)) material = m;
                done = true;
                lmask = lane_bits(kx, ky, kz);
            }
        }
        uint32_t vote = done ? VRT_VOTE_DONE : clear;
        asm volatile("" : "+v"(vote));
        if (__ballot(vote != VRT_VOTE_DONE) == 0ull) break;
        const float ox = s.sdx, oy = s.sdy, oz = s.sdz;
        if (__ballot(vote < 5u) != 0ull) {
            // a short run for everybody: the smallest clearance, 1..4 iterations, the last one's EXEC masks are the mask bits
            const uint32_t kw = wave_min_vote(vote);
            const uint64_t live = __ballot(vote != VRT_VOTE_DONE);
            float qx, qy, qz;
            dda_run_live_masks(s, live, kw, kx, ky, kz, qx, qy, qz);
        } else {
            // (a lane's own clearance, but no more than VRT_THRESH_SPREAD times the smallest of the wave: the others wait for the
            // lane that goes furthest; a finished lane has T = -1: it takes no step)
            const uint32_t kmin = wave_min_vote(vote), cap = kmin * (uint32_t)VRT_THRESH_SPREAD;
            const float cm1 = (float)((clear < cap ? clear : cap) - 1u);
            float T = fminf(fminf(__builtin_fmaf(cm1, s.dx, s.sdx), __builtin_fmaf(cm1, s.dy, s.sdy)), __builtin_fmaf(cm1, s.dz, s.sdz)) * 0.99998474f;
            if (done) T = -1.0f;
            axis_run(s.sdx, s.dx, T);
            axis_run(s.sdy, s.dy, T);
            axis_run(s.sdz, s.dz, T);
        }
        const int nx = steps_signed(s.sdx - ox, gx), ny = steps_signed(s.sdy - oy, gy), nz = steps_signed(s.sdz - oz, gz);
        s.mx += nx; s.my += ny; s.mz += nz;
        if (cnt) steps += (uint32_t)((nx < 0 ? -nx : nx) + (ny < 0 ? -ny : ny) + (nz < 0 ? -nz : nz));
    }
    finish(s, material, lmask, cnt ? (v.count_lookups != 0u ? bytes : steps + (material != 0u ? 1u : 0u)) : 0u, r);
}
#endif

template <class STATS, bool ANYHIT = false, bool CNT = false>
VRT_HD void trace_brick(const VolumeView& v, f3 start, f3 dir, uint32_t maxSteps, RayInt& r, STATS& stats)
{
    DdaState s;
    dda_entry(v, start, dir, s);
    if (wave_all(oob(v, s.mx, s.my, s.mz))) {
        s.dx = s.dy = s.dz = 0.0f; s.sdx = s.sdy = s.sdz = 0.0f; s.sx = s.sy = s.sz = 0;
        finish(s, 0u, s.mask, 0u, r);
        r.dbg0 = 1u; r.dbg1 = 0u;
        return;
    }
    dda_rest(dir, s);
#if defined(__HIP_DEVICE_COMPILE__)
    // the march without a budget for a wave none of whose rays can take maxSteps iterations (the bound of trace_df_fast)
    if (__builtin_amdgcn_readfirstlane((int)v.df_thresh) != 0) {
        const float bound = s.tspan * ((fabsf(dir.x) + fabsf(dir.y)) + fabsf(dir.z)) * 1.001f + 8.0f;
        if (__ballot(!oob(v, s.mx, s.my, s.mz) && !(bound < (float)maxSteps)) == 0ull) {
            brick_march_thresh<STATS, CNT>(v, s, dir, r, stats);
            return;
        }
    }
    asm volatile("" : "+v"(s.dx), "+v"(s.dy), "+v"(s.dz));
    uint64_t kx = __ballot((s.mask & 1u) != 0u), ky = __ballot((s.mask & 2u) != 0u), kz = __ballot((s.mask & 4u) != 0u);
    uint32_t lmask = s.mask;
#else
    bool k0 = (s.mask & 1u) != 0u, k1 = (s.mask & 2u) != 0u, k2 = (s.mask & 4u) != 0u;
#endif
    uint32_t material = 0, fetches = 0, lk_bytes = 0;
    bool done = oob(v, s.mx, s.my, s.mz);
    uint32_t clear = 63u;
    const uint32_t oct = (uint32_t)(s.sx > 0) | ((uint32_t)(s.sy > 0) << 1) | ((uint32_t)(s.sz > 0) << 2);
    const float kInf = u2f(0x7F800000u);
    const float gx = s.dx < kInf ? dir.x : 0.0f, gy = s.dy < kInf ? dir.y : 0.0f, gz = s.dz < kInf ? dir.z : 0.0f;
    uint32_t i = 0;
#if defined(VRT_TRACE_COUNTERS)
    uint32_t n_look = 0, n_occ = 0;                            // development: look-ups of this lane, and those inside occupied bricks
#endif
    for (;;) {
        if (!done) {
            if (i >= maxSteps) {
                done = true; fetches = i;
#if defined(__HIP_DEVICE_COMPILE__)
                lmask = lane_bits(kx, ky, kz);
#endif
            } else {
                uint32_t m = 0u;
                clear = brick_clear(v, s.mx, s.my, s.mz, oct, s.sx, s.sy, s.sz, m, CNT ? &lk_bytes : nullptr);
                st_lookup(stats);
#if defined(VRT_TRACE_COUNTERS)
                n_look++;
                {
                    const uint32_t bi_ = (uint32_t)((s.mx >> 3) + 1) + (uint32_t)(((s.my >> 3) + 1) * v.pbx) + (uint32_t)(((s.mz >> 3) + 1) * v.pbx * v.pby);
                    const uint64_t e_ = v.bentry[bi_];
                    if ((((uint32_t)(e_ >> 32) >> (oct * 4u)) & 15u) == 0u) n_occ++;
                }
#endif
                if (clear == 0u) {                             // solid, or the border: the ray has left the volume
                    if (oob(v, s.mx, s.my, s.mz)) fetches = i;
                    else { material = m; fetches = i + 1u; }
                    done = true;
#if defined(__HIP_DEVICE_COMPILE__)
                    lmask = lane_bits(kx, ky, kz);
#endif
                } else if (ANYHIT && clear >= maxSteps - i) {
                    // any-hit ray whose clearance covers the rest of its budget: a miss with fetches = maxSteps, no stepping
                    done = true; fetches = v.count_marched ? i : maxSteps;
                }
            }
        }
        uint32_t vote = done ? VRT_VOTE_DONE : clear;
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+v"(vote));
#endif
        uint32_t kw = wave_min_vote(vote);
        if (kw == VRT_VOTE_DONE) break;
        uint32_t left = maxSteps - i;
        kw = kw < left ? kw : left;
        st_jump(stats, kw > 4u ? 2 : 1);
#if defined(__HIP_DEVICE_COMPILE__)
        {
            const uint64_t live = __ballot(vote != VRT_VOTE_DONE);
            float ox, oy, oz;
            dda_run_live_masks(s, live, kw, kx, ky, kz, ox, oy, oz);
            s.mx += steps_signed(s.sdx - ox, gx); s.my += steps_signed(s.sdy - oy, gy); s.mz += steps_signed(s.sdz - oz, gz);
        }
#else
        if (!done) {
            const float ox = s.sdx, oy = s.sdy, oz = s.sdz;
            for (uint32_t j = 1; j < kw; j++) dda_advance(s);
            {
                uint32_t bx = f2u(s.sdx), by = f2u(s.sdy), bz = f2u(s.sdz);
                uint32_t mn = umin3(bx, by, bz);
                k0 = bx == mn; k1 = by == mn; k2 = bz == mn;
                s.sdx = k0 ? s.sdx + s.dx : s.sdx;
                s.sdy = k1 ? s.sdy + s.dy : s.sdy;
                s.sdz = k2 ? s.sdz + s.dz : s.sdz;
            }
            s.mx += steps_signed(s.sdx - ox, gx); s.my += steps_signed(s.sdy - oy, gy); s.mz += steps_signed(s.sdz - oz, gz);
        }
#endif
        i += kw;
    }
    if (CNT && v.count_lookups != 0u) fetches = lk_bytes;       // (VRT_FLAG_LOOKUP_COUNTS: the bytes the look-ups asked for)
#if defined(__HIP_DEVICE_COMPILE__)
    finish(s, material, lmask, fetches, r);
#if defined(VRT_TRACE_COUNTERS)
    r.dbg0 = n_look; r.dbg1 = n_occ;
#endif
#else
    finish(s, material, (uint32_t)k0 | ((uint32_t)k1 << 1) | ((uint32_t)k2 << 2), fetches, r);
#endif
}

// What a lane of the brick pool carries from one call of brick_ao_pool to the next: the ray it is on, or none (live = false)
struct BrickAoLane { DdaState s; float gx, gy, gz; uint32_t i, owner; bool live; };
#if defined(__HIP_DEVICE_COMPILE__)
// The brick march for rays that point every way (AO): every lane spends its own clearance, up to VRT_OWN_CAP iterations per
// look (df_any_loop's scheme in the generic loop: an iteration runs under the ballot of the lanes that have some left).
template <class STATS, bool CNT = false>
__device__ __forceinline__ void trace_brick_own(const VolumeView& v, f3 start, f3 dir, uint32_t maxSteps, RayInt& r, STATS& stats)
{
    DdaState s;
    dda_entry(v, start, dir, s);
    if (wave_all(oob(v, s.mx, s.my, s.mz))) {
        s.dx = s.dy = s.dz = 0.0f; s.sdx = s.sdy = s.sdz = 0.0f; s.sx = s.sy = s.sz = 0;
        finish(s, 0u, s.mask, 0u, r);
        return;
    }
    dda_rest(dir, s);
    asm volatile("" : "+v"(s.dx), "+v"(s.dy), "+v"(s.dz));
    uint32_t material = 0u, fetches = 0u, i = 0u, lk_bytes = 0u;             // i: iterations THIS lane has taken
    bool done = oob(v, s.mx, s.my, s.mz);
    const uint32_t oct = (uint32_t)(s.sx > 0) | ((uint32_t)(s.sy > 0) << 1) | ((uint32_t)(s.sz > 0) << 2);
    const float kInf = u2f(0x7F800000u);
    const float gx = s.dx < kInf ? dir.x : 0.0f, gy = s.dy < kInf ? dir.y : 0.0f, gz = s.dz < kInf ? dir.z : 0.0f;
    for (;;) {
        uint32_t own = 0u;
        if (!done) {
            if (i >= maxSteps) { done = true; fetches = i; }
            else {
                uint32_t m = 0u;
                const uint32_t clear = brick_clear(v, s.mx, s.my, s.mz, oct, s.sx, s.sy, s.sz, m, CNT ? &lk_bytes : nullptr);
                st_lookup(stats);
                if (clear == 0u) {
                    if (oob(v, s.mx, s.my, s.mz)) fetches = i;
                    else { material = m; fetches = i + 1u; }
                    done = true;
                } else if (clear >= maxSteps - i) { done = true; fetches = v.count_marched ? i : maxSteps; }
                else own = clear < (uint32_t)VRT_OWN_CAP_BRICK ? clear : (uint32_t)VRT_OWN_CAP_BRICK;
            }
        }
        if (__ballot(own != 0u) == 0ull) break;
        const float ox = s.sdx, oy = s.sdy, oz = s.sdz;
#pragma unroll
        for (uint32_t j = 0; j < (uint32_t)VRT_OWN_CAP_BRICK; j++) {
            const uint64_t mk = __ballot(own > j);
            if (mk == 0ull) break;
            dda_advance_live(s, mk);
        }
        s.mx += steps_signed(s.sdx - ox, gx); s.my += steps_signed(s.sdy - oy, gy); s.mz += steps_signed(s.sdz - oz, gz);
        i += own;
    }
    finish(s, material, s.mask, (CNT && v.count_lookups != 0u) ? lk_bytes : fetches, r);
}

// ---- the same pool for brick scenes (df_ao_pool_loop's scheme in the generic loop) ---------------------------------------------
// A ray of the pool: 13 dwords (sideDist, deltaDist, 1 / delta with its sign, mapPos, tag = column of its pixel | first clearance << 8), slot k
// at row q: q * 256 + k * 4; the two rows of counters behind them (3328: rays of the column's pixel that found a solid voxel; 3584, CNT:
// what the count planes report).
__device__ __forceinline__ void brick_ao_rest(BrickAoLane& l)
{
    l.s.sdx = l.s.sdy = l.s.sdz = 0.0f; l.s.dx = l.s.dy = l.s.dz = 0.0f; l.s.mx = l.s.my = l.s.mz = 0; l.s.sx = l.s.sy = l.s.sz = 0;
    l.gx = l.gy = l.gz = 0.0f; l.i = 0u; l.owner = 0u; l.live = false;
}
// the set-up of the lane's pixel's next AO ray (frag:109-144) ...
__device__ __forceinline__ void brick_ao_setup(const VolumeView& v, f3 start, f3 dir, DdaState& s, float& gx, float& gy, float& gz)
{
    dda_entry(v, start, dir, s);
    dda_rest(dir, s);
    const float kInf = u2f(0x7F800000u);
    gx = s.dx < kInf ? dir.x : 0.0f; gy = s.dy < kInf ? dir.y : 0.0f; gz = s.dz < kInf ? dir.z : 0.0f;
}
// ... and the ray into slot `slot` of the pool; tag: the column of its pixel's counters | the clearance its owner read at its first voxel << 8
__device__ __forceinline__ void brick_ao_store(uint32_t ldsw, uint32_t slot, const DdaState& s, float gx, float gy, float gz, uint32_t tag)
{
    __attribute__((address_space(3))) uint32_t* p = (__attribute__((address_space(3))) uint32_t*)(uintptr_t)(ldsw + slot * 4u);
    p[0 * 64] = f2u(s.sdx); p[1 * 64] = f2u(s.sdy); p[2 * 64] = f2u(s.sdz);
    p[3 * 64] = f2u(s.dx); p[4 * 64] = f2u(s.dy); p[5 * 64] = f2u(s.dz);
    p[6 * 64] = f2u(gx); p[7 * 64] = f2u(gy); p[8 * 64] = f2u(gz);
    p[9 * 64] = (uint32_t)s.mx; p[10 * 64] = (uint32_t)s.my; p[11 * 64] = (uint32_t)s.mz; p[12 * 64] = tag;
}
// One call: `count` rays wait in the pool, `next` of them are taken (in / out); more: come back when the pool is empty and a lane
// rests.  Every lane spends its ray's own clearance, at most VRT_OWN_CAP_BRICK iterations per look (trace_brick_own).
template <bool CNT>
__device__ __forceinline__ void brick_ao_pool(const VolumeView& v, BrickAoLane& l, uint32_t ldsw, uint32_t count, bool more, uint32_t& next,
                                              uint32_t maxSteps, uint32_t& looks)
{
    __attribute__((address_space(3))) uint32_t* pool = (__attribute__((address_space(3))) uint32_t*)(uintptr_t)ldsw;
    for (;;) {
        uint32_t own = 0u;
        if (l.live) {
            bool ended = false, solid = false;
            uint32_t fet = 0u;
            if (l.i >= maxSteps) { ended = true; fet = l.i; }
            else {
                const uint32_t oct = (uint32_t)(l.s.sx > 0) | ((uint32_t)(l.s.sy > 0) << 1) | ((uint32_t)(l.s.sz > 0) << 2);
                uint32_t m = 0u;
                const uint32_t clear = brick_clear(v, l.s.mx, l.s.my, l.s.mz, oct, l.s.sx, l.s.sy, l.s.sz, m, CNT ? &looks : nullptr);
                if (clear == 0u) {
                    ended = true;
                    solid = !oob(v, l.s.mx, l.s.my, l.s.mz) && m != 0u;
                    fet = solid ? l.i + 1u : l.i;
                } else if (clear >= maxSteps - l.i) { ended = true; fet = v.count_marched ? l.i : maxSteps; }
                else own = clear < (uint32_t)VRT_OWN_CAP_BRICK ? clear : (uint32_t)VRT_OWN_CAP_BRICK;
            }
            if (ended) {
                if (solid) __hip_atomic_fetch_add(pool + 13 * 64 + l.owner, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (CNT) __hip_atomic_fetch_add(pool + 14 * 64 + l.owner, fet, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                l.live = false;
            }
        }
        // lanes without a ray take the next ones of the pool: the wave's counter + the lane's rank among those asking
        const uint64_t asking = __ballot(!l.live);
        if (!l.live) {
            const uint32_t slot = next + __builtin_amdgcn_mbcnt_hi((uint32_t)(asking >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)asking, 0u));
            if (slot < count) {
                __attribute__((address_space(3))) uint32_t* p = pool + slot;
                l.s.sdx = u2f(p[0 * 64]); l.s.sdy = u2f(p[1 * 64]); l.s.sdz = u2f(p[2 * 64]);
                l.s.dx = u2f(p[3 * 64]); l.s.dy = u2f(p[4 * 64]); l.s.dz = u2f(p[5 * 64]);
                l.gx = u2f(p[6 * 64]); l.gy = u2f(p[7 * 64]); l.gz = u2f(p[8 * 64]);
                l.s.mx = (int)p[9 * 64]; l.s.my = (int)p[10 * 64]; l.s.mz = (int)p[11 * 64];
                // rayStep from the direction's signs (an axis the ray cannot step along has g = 0: the step is never taken)
                l.s.sx = l.gx > 0.0f ? 1 : (l.gx < 0.0f ? -1 : 0); l.s.sy = l.gy > 0.0f ? 1 : (l.gy < 0.0f ? -1 : 0); l.s.sz = l.gz > 0.0f ? 1 : (l.gz < 0.0f ? -1 : 0);
                const uint32_t tag = p[12 * 64];
                l.i = 0u; l.owner = tag & 0xFFu; l.live = true;
                // (its owner read the clearance at its first voxel: 1 .. maxSteps - 1; the lane marches it in this very round)
                const uint32_t c0 = tag >> 8;
                own = c0 < (uint32_t)VRT_OWN_CAP_BRICK ? c0 : (uint32_t)VRT_OWN_CAP_BRICK;
            }
        }
        const uint32_t taken = next + (uint32_t)__builtin_popcountll(asking);
        next = taken < count ? taken : count;
        const uint64_t live = __ballot(l.live);
        if (next >= count && more && __ballot(!l.live) != 0ull) return;      // the pool wants refilling
        if (live == 0ull) return;
        if (__ballot(own != 0u) == 0ull) continue;                          // (only rays just taken up: their first look)
        const float ox = l.s.sdx, oy = l.s.sdy, oz = l.s.sdz;
        asm volatile("" : "+v"(l.s.dx), "+v"(l.s.dy), "+v"(l.s.dz));
#pragma unroll
        for (uint32_t j = 0; j < (uint32_t)VRT_OWN_CAP_BRICK; j++) {
            const uint64_t mk = __ballot(own > j);
            if (mk == 0ull) break;
            dda_advance_live(l.s, mk);
        }
        l.s.mx += steps_signed(l.s.sdx - ox, l.gx); l.s.my += steps_signed(l.s.sdy - oy, l.gy); l.s.mz += steps_signed(l.s.sdz - oz, l.gz);
        l.i += own;
    }
}
#endif

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- HOST STUBS of this header's device-only functions -----------------------------------------------------------
// host pass of a .hip file / the host build of the unit tests: parsed, never run (the loop is gfx950 assembly)
template <class STATS, bool CNT = false>
VRT_HD void trace_brick_own(const VolumeView&, f3, f3, uint32_t, RayInt&, STATS&) {}
VRT_HD void brick_ao_rest(BrickAoLane&) {}
VRT_HD void brick_ao_setup(const VolumeView&, f3, f3, DdaState&, float&, float&, float&) {}
VRT_HD void brick_ao_store(uint32_t, uint32_t, const DdaState&, float, float, float, uint32_t) {}
template <bool CNT> VRT_HD void brick_ao_pool(const VolumeView&, BrickAoLane&, uint32_t, uint32_t, bool, uint32_t&, uint32_t, uint32_t&) {}
#endif

} // namespace vrt
