// vrt_march_df.h -- DF in plain C++: trace_df_impl, the wave-cooperative clearance-field march that every other DF form is
// measured against bit for bit, and trace_df, its entry.  Included by vrt_traverse.h (the dispatch) and by
// vrt_march_literal.h (trace_dfj re-traces through trace_df).  No assembly beyond empty register-pinning statements; the
// same code runs on the host in the unit tests.
#pragma once

#include "vrt_dda.h"     // (over vrt_volume.h: the data types and the DDA)

namespace vrt {

// ---- DF in plain C++ -----------------------------------------------------------------------------------------

// DF (clearance-field skip, wave-cooperative).  Profiling showed the per-iteration loops are bound by the
// vector-memory pipe and by instruction issue, not by arithmetic: one 64-lane byte gather per DDA iteration
// touches ~24 cache lines on the bench frame and sits on the critical path of every iteration.  Here a set of
// byte volumes holds, per empty voxel and per direction octant, the side k of the largest empty cube that has
// the voxel as its corner and extends towards the octant's signs.  A ray only ever moves towards the signs of
// its direction, at most one voxel per axis per DDA iteration, so its next k-1 iterations stay inside that cube:
// no memory test is needed for them (unlike an isotropic distance field, the clearance of a ray LEAVING a
// surface is large at once).  Voxels outside the volume count as solid, which bounds a run at the walls.  The lanes of a wave agree on the smallest clearance among them (wave_min_vote) and run
// that many iterations of pure ALU stepping -- the same fp32 additions as the shader, hence bit-identical
// results -- then look at memory again.  Neighbouring rays have similar clearances, so the wave-wide minimum
// costs little.  Finished lanes are masked off; the votes see live lanes only.
template <bool SMALL, class STATS, bool AHEAD>
VRT_HD void trace_df_impl(const VolumeView& v, f3 start, f3 dir, uint32_t maxSteps, RayInt& r, STATS& stats)
{
    DdaState s;
    dda_entry(v, start, dir, s);
    // A ray that starts outside the volume and misses it begins the loop at its own origin (frag:118-126) and leaves in
    // iteration 0.  When that is every lane of the wave -- the sky tiles of a frame -- the rest of the set-up, the
    // look-up and the vote have nothing to decide.
    if (wave_all(oob(v, s.mx, s.my, s.mz))) {
        s.dx = s.dy = s.dz = 0.0f; s.sdx = s.sdy = s.sdz = 0.0f; s.sx = s.sy = s.sz = 0;
        finish(s, 0u, s.mask, 0u, r);
        r.dbg0 = 1u; r.dbg1 = 0u;
        return;
    }
    dda_rest(dir, s);
#if defined(__HIP_DEVICE_COMPILE__)
    // deltaDist = |1/dir|: keep the three values in registers of their own (otherwise the |.| is rematerialised as
    // an extra VALU op in every iteration of the stepping loop, whose asm operands cannot take source modifiers)
    asm volatile("" : "+v"(s.dx), "+v"(s.dy), "+v"(s.dz));
#endif
    uint32_t material = 0, fetches = 0;
    // the mask of the latest iteration, one bool per axis: the compiler keeps each as a 64-bit lane mask in scalar
    // registers (the compare results themselves), so recording it costs no vector instructions
    // (device: three wave-wide lane masks, updated by the EXEC masks of the run's last iteration -- scalar moves only)
#if defined(__HIP_DEVICE_COMPILE__)
    // kx/ky/kz: the EXEC masks of the latest run's last iteration (the mask bits of the lanes that were live in it); a lane
    // copies its bits out when it finishes (lmask) -- five vector instructions in the hit path instead of six scalar ones
    // per look-up to keep three merged wave-wide masks up to date
    uint64_t kx = __ballot((s.mask & 1u) != 0u), ky = __ballot((s.mask & 2u) != 0u), kz = __ballot((s.mask & 4u) != 0u);
    uint32_t lmask = s.mask;
#else
    bool k0 = (s.mask & 1u) != 0u, k1 = (s.mask & 2u) != 0u, k2 = (s.mask & 4u) != 0u;
#endif
    // a ray that starts outside the volume and misses it begins the loop at its own origin (frag:118-126) and leaves
    // in iteration 0; every later position is inside the volume or in the one-voxel border of the fields
    bool done = oob(v, s.mx, s.my, s.mz);
    uint32_t clear = 63u;
    // clearance field of the octant the ray travels into (an axis the ray does not move along can use either sign)
    const uint32_t oct = (uint32_t)(s.sx > 0) | ((uint32_t)(s.sy > 0) << 1) | ((uint32_t)(s.sz > 0) << 2);
    // index into the padded field, kept incrementally; IDX is 32 bits while all eight fields stay below 4 GiB
    typedef typename IndexT<SMALL>::type IDX;
    typedef typename IndexT<SMALL>::stype SIDX;
    const int pw = v.W + 2;
    const long long pwh = (long long)pw * (long long)(v.H + 2);
    IDX idx = done ? (IDX)0 : (IDX)((size_t)oct * (size_t)v.df_stride + df_index(v, s.mx, s.my, s.mz));
    const float kInf = u2f(0x7F800000u);
    // signed steps per unit of sideDist: dir is 1/(+-delta) to within an ulp; 0 for an axis that cannot step
    const float gx = s.dx < kInf ? dir.x : 0.0f, gy = s.dy < kInf ? dir.y : 0.0f, gz = s.dz < kInf ? dir.z : 0.0f;
    uint32_t i = 0;                                            // wave-uniform: every live lane has done i iterations
    // look-ups and iterations in runs of >= 12: host instrumentation; on the device only in development builds
    // (make HIPFLAGS+=-DVRT_TRACE_COUNTERS for tools/exp_wavecost.py, exp_skipstats.py) -- four scalar instructions per
    // look-up in a kernel whose scalar unit is not idle
#if !defined(__HIP_DEVICE_COMPILE__) || defined(VRT_TRACE_COUNTERS)
#define VRT_DF_COUNT(x) x
#else
#define VRT_DF_COUNT(x)
#endif
    VRT_DF_COUNT(uint32_t n_outer = 0; uint32_t n_long = 0;)
#if defined(__HIP_DEVICE_COMPILE__)
    // the clearance of the next look-up is requested as soon as its index is known, at the end of the loop body, by every
    // lane (a finished lane re-reads the byte it stopped at): the mask merges, position updates and the loop's scalar
    // bookkeeping then run while the byte is on its way instead of before the request.  AHEAD: primary rays of the
    // primary-only kernel; in the megakernel the extra request per ray costs the short secondary rays more than it hides
    // (+15 % on the reference defaults).
    uint32_t ahead = AHEAD ? v.df[idx] : 0u;
    if (AHEAD && maxSteps == 0u) done = true;                  // (fetches = 0: no iteration runs)
#endif
    for (;;) {
        VRT_DF_COUNT(n_outer++;)
#if defined(__HIP_DEVICE_COMPILE__)
        // Flat form: the budget test is wave-uniform (i is), every lane takes the byte, and only the lanes that found 0
        // enter divergent code -- not a divergent `if (!done)` around everything, whose EXEC bookkeeping is a dozen scalar
        // instructions per look-up.
        // (Primary rays of the primary-only kernel, like the look-ahead request: the megakernel loses 10 % with it.)
        uint32_t vote;
        if (AHEAD) {                                           // i < maxSteps here: the budget is tested where i grows
            clear = ahead;
            st_lookup(stats);
            // the vote value first: a live lane that found 0 is the one lane whose vote is 0, so "did anybody hit" is one
            // compare and a wave-uniform branch that falls through when nobody did (no s_and_saveexec / taken branch /
            // s_or exec around a divergent region in the common case)
            vote = done ? VRT_VOTE_DONE : clear;
            asm volatile("" : "+v"(vote));
            if (__builtin_expect(__ballot(vote == 0u) != 0ull, 0)) {
                if (vote == 0u) {                              // solid, or the border: the ray has left the volume
                    if (oob(v, s.mx, s.my, s.mz)) fetches = i;
                    else {
                        material = SMALL ? v.vox[(uint32_t)s.mx + ((uint32_t)s.my + (uint32_t)s.mz * (uint32_t)v.H) * (uint32_t)v.W]
                                         : voxel_at(v, s.mx, s.my, s.mz);
                        fetches = i + 1u;
                    }
                    done = true;
                    lmask = lane_bits(kx, ky, kz);
                    vote = VRT_VOTE_DONE;
                }
            }
        } else if (!done) {
            if (i >= maxSteps) { done = true; fetches = i; lmask = lane_bits(kx, ky, kz); }
            else {
                clear = v.df[idx];
                st_lookup(stats);
                if (clear == 0u) {
                    if (oob(v, s.mx, s.my, s.mz)) fetches = i;
                    else {
                        material = SMALL ? v.vox[(uint32_t)s.mx + ((uint32_t)s.my + (uint32_t)s.mz * (uint32_t)v.H) * (uint32_t)v.W]
                                         : voxel_at(v, s.mx, s.my, s.mz);
                        fetches = i + 1u;
                    }
                    done = true;
                    lmask = lane_bits(kx, ky, kz);
                }
            }
        }
#else
        if (!done) {
            if (i >= maxSteps) { done = true; fetches = i; }
            else {
                clear = v.df[idx];
                st_lookup(stats);
                if (clear == 0u) {                             // solid, or the border: the ray has left the volume
                    if (oob(v, s.mx, s.my, s.mz)) fetches = i;
                    else {
                        material = SMALL ? v.vox[(uint32_t)s.mx + ((uint32_t)s.my + (uint32_t)s.mz * (uint32_t)v.H) * (uint32_t)v.W]
                                         : voxel_at(v, s.mx, s.my, s.mz);
                        fetches = i + 1u;
                    }
                    done = true;
                }
            }
        }
#endif
        // iterations the wave can take blind: the smallest clearance among its live lanes (the fields count the
        // outside of the volume as solid, so a run cannot carry a lane further than one voxel past a wall); the same
        // vote says whether anybody is still live
#if defined(__HIP_DEVICE_COMPILE__)
        if (!AHEAD) vote = done ? VRT_VOTE_DONE : clear;               // live lanes stand on empty in-bounds voxels: >= 1
        asm volatile("" : "+v"(vote));                                 // (keeps the compare below a compare: see `live`)
#else
        uint32_t vote = done ? VRT_VOTE_DONE : clear;
#endif
        uint32_t kw = wave_min_vote(vote);
        if (kw == VRT_VOTE_DONE) break;
        uint32_t left = maxSteps - i;                          // i < maxSteps for every live lane
        kw = kw < left ? kw : left;
        st_jump(stats, kw > 4u ? 2 : 1);
        VRT_DF_COUNT(if (kw >= 12u) n_long += kw;)
#if defined(__HIP_DEVICE_COMPILE__)
        {
            // The run is wave-uniform control flow: every lane executes it, but the stepping asm narrows EXEC to the live
            // lanes itself, so a finished lane's sideDist stands still, its differences below are 0 and its mapPos /
            // index do not move.  (Inside a divergent `if (!done)` the three lane masks would be per-lane values: six
            // VGPRs and twelve VALU ops per look-up to merge them.)
            const uint64_t live = __ballot(vote != VRT_VOTE_DONE);     // one compare; __ballot(!done) of the bool is two ops + a scalar one
            // Only sideDist is advanced inside the run; mapPos is recovered afterwards: an axis that took n steps has
            // grown by n (+) additions of delta, so n = round((side - side_before) / delta) -- n <= 63 per run and the
            // accumulated rounding error is orders of magnitude below 1/2.
            float ox, oy, oz;
            // kw - 1 iterations whose mask nobody will read, then one whose EXEC masks are the mask bits
            dda_run_live_masks(s, live, kw, kx, ky, kz, ox, oy, oz);
            const int nx = steps_signed(s.sdx - ox, gx), ny = steps_signed(s.sdy - oy, gy), nz = steps_signed(s.sdz - oz, gz);
            idx += SMALL ? (IDX)(nx + mul24(ny, pw) + mul24(nz, (int)pwh))
                         : (IDX)((SIDX)nx + (SIDX)ny * (SIDX)pw + (SIDX)nz * (SIDX)pwh);
            if (AHEAD) ahead = v.df[idx];
            s.mx += nx; s.my += ny; s.mz += nz;
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
            const int nx = steps_signed(s.sdx - ox, gx), ny = steps_signed(s.sdy - oy, gy), nz = steps_signed(s.sdz - oz, gz);
            s.mx += nx; s.my += ny; s.mz += nz;
            idx += SMALL ? (IDX)(nx + mul24(ny, pw) + mul24(nz, (int)pwh))
                         : (IDX)((SIDX)nx + (SIDX)ny * (SIDX)pw + (SIDX)nz * (SIDX)pwh);
        }
#endif
        i += kw;
#if defined(__HIP_DEVICE_COMPILE__)
        if (AHEAD && i >= maxSteps) {                          // wave-uniform: the budget ends for every live lane at once
            if (!done) { fetches = i; lmask = lane_bits(kx, ky, kz); }
            break;
        }
#endif
    }
#if defined(__HIP_DEVICE_COMPILE__)
    finish(s, material, lmask, fetches, r);
#else
    finish(s, material, (uint32_t)k0 | ((uint32_t)k1 << 1) | ((uint32_t)k2 << 2), fetches, r);
#endif
    VRT_DF_COUNT(r.dbg0 = n_outer; r.dbg1 = n_long;)
#undef VRT_DF_COUNT
}

template <class STATS, bool AHEAD = false>
VRT_HD void trace_df(const VolumeView& v, f3 start, f3 dir, uint32_t maxSteps, RayInt& r, STATS& stats)
{
    // wave-uniform choice; the 64-bit variant is only reached by volumes whose eight fields total 4 GiB or more (or
    // whose padded z-slice does not fit the 24-bit multiply of the incremental index)
    if (df_small(v)) trace_df_impl<true, STATS, AHEAD>(v, start, dir, maxSteps, r, stats);
    else trace_df_impl<false, STATS, AHEAD>(v, start, dir, maxSteps, r, stats);
}

} // namespace vrt
