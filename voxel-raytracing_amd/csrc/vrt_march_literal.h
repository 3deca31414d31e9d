// vrt_march_literal.h -- the literal strategies: DENSE (trace_dense, trace_dense_blocked), BITMASK, trace_literal over
// them, and the exact jumps (the essay, JumpAxis / jump_axis_*, trace_jump, trace_dfj).  Included by vrt_traverse.h.
// Plain C++ for host and device alike, no assembly, no host stubs.
#pragma once

#include "vrt_dda.h"     // (over vrt_volume.h: the data types and the DDA)
#include "vrt_march_df.h"     // (trace_dfj decides its ambiguous rays through trace_df)

namespace vrt {

// DENSE: one R8 fetch per iteration.  Straight-line body with a single exit (out of budget, out of bounds or
// solid), the voxel index maintained incrementally in IDX (uint32_t for volumes below 4 GiB).
template <class IDX>
VRT_HD void trace_dense(const VolumeView& v, f3 start, f3 dir, uint32_t maxSteps, RayInt& r)
{
    DdaState s;
    dda_setup(v, start, dir, s);
    uint32_t mask = s.mask, material = 0, i = 0;
    IDX idx = (IDX)s.mx + (IDX)s.my * (IDX)v.W + (IDX)s.mz * (IDX)v.W * (IDX)v.H;   // meaningless (and unused) while out of bounds
    const IDX incx = (IDX)(int64_t)s.sx, incy = (IDX)((int64_t)s.sy * (int64_t)v.W),
              incz = (IDX)((int64_t)s.sz * (int64_t)v.W * (int64_t)v.H);
    for (;;) {
        bool stop = i >= maxSteps || oob(v, s.mx, s.my, s.mz);
        uint32_t m = v.vox[stop ? (IDX)0 : idx];
        if (stop || m != 0u) { material = stop ? 0u : m; break; }
        ++i;
        uint32_t bx = f2u(s.sdx), by = f2u(s.sdy), bz = f2u(s.sdz);
        uint32_t mn = umin3(bx, by, bz);
        bool m0 = bx == mn, m1 = by == mn, m2 = bz == mn;
        mask = (uint32_t)m0 | ((uint32_t)m1 << 1) | ((uint32_t)m2 << 2);
        s.sdx = m0 ? s.sdx + s.dx : s.sdx; s.mx += m0 ? s.sx : 0;
        s.sdy = m1 ? s.sdy + s.dy : s.sdy; s.my += m1 ? s.sy : 0;
        s.sdz = m2 ? s.sdz + s.dz : s.sdz; s.mz += m2 ? s.sz : 0;
        idx += (m0 ? incx : (IDX)0) + (m1 ? incy : (IDX)0) + (m2 ? incz : (IDX)0);
    }
    finish(s, material, mask, material ? i + 1u : i, r);
}

// DENSE, latency-hiding form.  The DDA advance does not depend on the fetched voxel -- only the exit test
// does -- so the march runs B iterations ahead with B fetches in flight, then looks for the first iteration
// that should have stopped; if there is one, the saved state is replayed up to it with the same arithmetic.
// One fetch latency (an L2 / Infinity-Cache hit, 200-550 cycles) is paid per B iterations instead of per
// iteration; this is what shortens the critical path of the longest ray in a frame.
template <int B>
VRT_HD void trace_dense_blocked(const VolumeView& v, f3 start, f3 dir, uint32_t maxSteps, RayInt& r)
{
    DdaState s;
    dda_setup(v, start, dir, s);
    uint32_t mask = s.mask, material = 0, i = 0;
    uint32_t idx = (uint32_t)s.mx + (uint32_t)s.my * (uint32_t)v.W + (uint32_t)s.mz * (uint32_t)v.W * (uint32_t)v.H;
    const uint32_t incx = (uint32_t)s.sx, incy = (uint32_t)(s.sy * v.W), incz = (uint32_t)(s.sz * v.W * v.H);
    for (;;) {
        // snapshot
        const float s0x = s.sdx, s0y = s.sdy, s0z = s.sdz;
        const int m0x = s.mx, m0y = s.my, m0z = s.mz;
        const uint32_t mask0 = mask;
        uint32_t vox[B];
        uint32_t stopbits = 0;
#pragma unroll
        for (int b = 0; b < B; b++) {
            bool stop = (i + (uint32_t)b) >= maxSteps || oob(v, s.mx, s.my, s.mz);
            stopbits |= (uint32_t)stop << b;
            vox[b] = v.vox[stop ? 0u : idx];
            uint32_t bx = f2u(s.sdx), by = f2u(s.sdy), bz = f2u(s.sdz);
            uint32_t mn = umin3(bx, by, bz);
            bool k0 = bx == mn, k1 = by == mn, k2 = bz == mn;
            mask = (uint32_t)k0 | ((uint32_t)k1 << 1) | ((uint32_t)k2 << 2);
            s.sdx = k0 ? s.sdx + s.dx : s.sdx; s.mx += k0 ? s.sx : 0;
            s.sdy = k1 ? s.sdy + s.dy : s.sdy; s.my += k1 ? s.sy : 0;
            s.sdz = k2 ? s.sdz + s.dz : s.sdz; s.mz += k2 ? s.sz : 0;
            idx += (k0 ? incx : 0u) + (k1 ? incy : 0u) + (k2 ? incz : 0u);
        }
        uint32_t exitbits = stopbits;
#pragma unroll
        for (int b = 0; b < B; b++) exitbits |= (uint32_t)(vox[b] != 0u) << b;
        if (exitbits == 0u) { i += (uint32_t)B; continue; }
        // first iteration of the block that stops: replay the snapshot up to it
        int first = 0;
#pragma unroll
        for (int b = B - 1; b >= 0; b--) if ((exitbits >> b) & 1u) first = b;
        uint32_t m = 0;
#pragma unroll
        for (int b = 0; b < B; b++) if (b == first) m = vox[b];
        material = ((stopbits >> first) & 1u) ? 0u : m;
        s.sdx = s0x; s.sdy = s0y; s.sdz = s0z; s.mx = m0x; s.my = m0y; s.mz = m0z; mask = mask0;
        for (int b = 0; b < first; b++) VRT_DDA_STEP(s, mask);
        i += (uint32_t)first;
        break;
    }
    finish(s, material, mask, material ? i + 1u : i, r);
}

template <int TRAV, class OP>
VRT_HD void trace_literal(const VolumeView& v, OP o2, f3 start, f3 dir, uint32_t maxSteps, RayInt& r)
{
    if (TRAV == VRT_TRAVERSAL_DENSE) {
        trace_dense_blocked<4>(v, start, dir, maxSteps, r);    // the API rejects DENSE for volumes of 4 GiB and more
        return;
    }
    DdaState s;
    dda_setup(v, start, dir, s);
    uint32_t mask = s.mask, material = 0, fetches = 0;
    uint32_t ckey = 0xFFFFFFFFu;
    uint64_t word = 0;
    uint32_t i = 0;
    for (; i < maxSteps; i++) {
        if (oob(v, s.mx, s.my, s.mz)) break;
        uint32_t key = (uint32_t)(s.mx >> 2) | ((uint32_t)(s.my >> 2) << 10) | ((uint32_t)(s.mz >> 2) << 20);
        if (key != ckey) { ckey = key; word = fetch_cell(v, o2, s.mx >> 2, s.my >> 2, s.mz >> 2); }
        if ((word >> cell_bit(s.mx, s.my, s.mz)) & 1ull) {
            material = voxel_at(v, s.mx, s.my, s.mz);
            fetches = i + 1;
            break;
        }
        VRT_DDA_STEP(s, mask);
    }
    if (material == 0) fetches = i;
    finish(s, material, mask, fetches, r);
}

// ---- exact jumps ----------------------------------------------------------------------------------------
// The shader advances sideDist by repeated fp32 addition (frag:167), so after k steps along an axis
// sideDist = s (+) d (+) d ... (k roundings), which is not s + k*d.  Within one binade of s, however,
// RN(s + d) = s + Q*ulp(s) for a constant integer Q (d rounded to the ulp of s; a half-ulp tie rounds to
// even and, once the mantissa is even, keeps it even), and the bit pattern of a positive float is monotone
// in its value.  Hence, on the bit patterns, k additions are ONE integer multiply-add, S(j) = bits + j*Q,
// valid until the mantissa would overflow into the next binade.  The DDA's interleaving of the three
// axes is a merge of three such arithmetic sequences by value, ties stepping together (frag:164), so the
// state after any number of iterations is computable in closed form:
//   n_a  = steps axis a may take before leaving the empty cell (or the binade), T_a = S_a(n_a - 1)
//   T*   = min T_a: the sideDist value at which the last iteration of the jump happens
//   c_a  = n_a for the axes with T_a == T*, else #{j : S_a(j) <= T*} = floor((T* - bits_a)/Q_a) + 1
//   mask = axes whose last step was taken exactly at T*
// The final addition of every axis that reaches T* is performed in fp32, so binade crossings are literal.
// The iteration budget (MAX_RAY_STEPS) is tracked as bounds: every iteration steps 1..3 axes, so
// max_a(steps_a) <= iterations <= sum_a(steps_a); a hit whose bounds straddle the budget (only possible
// for rays with exact ties that run within a few steps of the budget) is re-traced literally.

// Increment of the bit pattern per addition of d while the sum stays in the binade of `bits`, and how many
// further additions are guaranteed to stay there (conservative).  false: no closed form here (zero/denormal/
// inf sideDist, d not below the binade of s, or a half-ulp tie on an odd mantissa) -> step that axis literally.
VRT_HD bool axis_increment(uint32_t bits, float d, uint32_t& Q, uint32_t& jmax)
{
    uint32_t db = f2u(d);
    uint32_t E = bits >> 23, Ed = db >> 23;
    int shift = (int)E - (int)Ed;
    if (E == 0u || E >= 255u || shift < 1 || shift > 20) return false;
    uint32_t Md = (db & 0x7FFFFFu) | 0x800000u;
    uint32_t q = Md >> shift;
    uint32_t rem = Md & ((1u << shift) - 1u), half = 1u << (shift - 1);
    if (rem > half) q += 1u;
    else if (rem == half) { if (bits & 1u) return false; q += (q & 1u); }
    uint32_t room = 0xFFFFFFu - ((bits & 0x7FFFFFu) | 0x800000u);       // mantissa head-room in this binade
    uint32_t je = (uint32_t)((float)room * rcp_approx((float)q));
    jmax = je > 0u ? je - 1u : 0u;                                       // conservative: never over-estimates
    Q = q;
    return true;
}

struct JumpAxis { uint32_t bits, Q, T; int n; };

VRT_HD void jump_axis_prepare(float side, float d, int step, int n_region, JumpAxis& a)
{
    a.bits = f2u(side);
    a.Q = 0u;
    if (step == 0) { a.n = 0; a.T = 0xFFFFFFFFu; return; }
    uint32_t jmax;
    if (axis_increment(a.bits, d, a.Q, jmax)) {
        int lim = (int)jmax + 1;
        a.n = n_region < lim ? n_region : lim;
    } else {
        a.n = 1; a.Q = 0u;
    }
    a.T = a.bits + (uint32_t)(a.n - 1) * a.Q;
}

// Advance axis by the steps it takes up to and including time T*.  Returns the number of steps; `last` tells
// whether its final step happened exactly at T* (it then belongs to the final iteration's mask).
VRT_HD int jump_axis_apply(const JumpAxis& a, uint32_t Tstar, float d, float& side, bool& last)
{
    last = false;
    if (a.n == 0) return 0;
    if (a.T == Tstar) {                                   // reaches its n-th step at T*: last addition in fp32
        side = u2f(a.T) + d;
        last = true;
        return a.n;
    }
    if (a.Q == 0u || Tstar < a.bits) return 0;
    uint32_t num = Tstar - a.bits;
    uint32_t c = (uint32_t)((float)num * rcp_approx((float)a.Q));
    if (c * a.Q > num) c -= 1u;
    else if ((c + 1u) * a.Q <= num) c += 1u;
    last = (c * a.Q == num);
    c += 1u;                                              // steps j = 0..c-1 have S(j) <= T*
    side = u2f(a.bits + c * a.Q);
    return (int)c;
}

VRT_HD int iabs(int x) { return x < 0 ? -x : x; }

template <class STATS, class OP>
VRT_HD void trace_jump(const VolumeView& v, OP o2, OP o3, f3 start, f3 dir,
                       uint32_t maxSteps, RayInt& r, STATS& stats)
{
    DdaState s;
    dda_setup(v, start, dir, s);
    const int mx0 = s.mx, my0 = s.my, mz0 = s.mz;
    uint32_t mask = s.mask, material = 0;
    uint32_t it_up = 0;                                   // upper bound of DDA iterations done (sum of axis steps)
    uint32_t ckey = 0xFFFFFFFFu;
    uint64_t word = 0;
    int lvl = 0;
    bool hit = false;
    for (;;) {
        if (oob(v, s.mx, s.my, s.mz)) break;
        uint32_t key = (uint32_t)(s.mx >> 2) | ((uint32_t)(s.my >> 2) << 10) | ((uint32_t)(s.mz >> 2) << 20);
        if (key != ckey) { ckey = key; lvl = lookup_level(v, o2, o3, s.mx, s.my, s.mz, word); st_lookup(stats); }
        if (lvl == 0) {
            if ((word >> cell_bit(s.mx, s.my, s.mz)) & 1ull) { hit = true; break; }
            VRT_DDA_STEP(s, mask);
            it_up += (mask & 1u) + ((mask >> 1) & 1u) + ((mask >> 2) & 1u);
            st_literal(stats);
        } else {
            // empty aligned cell of edge sz around mapPos, clipped to the volume
            int sh = 2 * lvl, sz = 1 << sh;
            int lox = (s.mx >> sh) << sh, loy = (s.my >> sh) << sh, loz = (s.mz >> sh) << sh;
            int hix = lox + sz < v.W ? lox + sz : v.W;
            int hiy = loy + sz < v.H ? loy + sz : v.H;
            int hiz = loz + sz < v.D ? loz + sz : v.D;
            JumpAxis ax, ay, az;
            jump_axis_prepare(s.sdx, s.dx, s.sx, s.sx > 0 ? hix - s.mx : s.mx - lox + 1, ax);
            jump_axis_prepare(s.sdy, s.dy, s.sy, s.sy > 0 ? hiy - s.my : s.my - loy + 1, ay);
            jump_axis_prepare(s.sdz, s.dz, s.sz, s.sz > 0 ? hiz - s.mz : s.mz - loz + 1, az);
            uint32_t Tstar = ax.T < ay.T ? ax.T : ay.T;
            Tstar = Tstar < az.T ? Tstar : az.T;
            if (Tstar == 0xFFFFFFFFu) break;              // direction (0,0,0): the literal loop spins to the budget -> miss
            bool l0, l1, l2;
            int c0 = jump_axis_apply(ax, Tstar, s.dx, s.sdx, l0);
            int c1 = jump_axis_apply(ay, Tstar, s.dy, s.sdy, l1);
            int c2 = jump_axis_apply(az, Tstar, s.dz, s.sdz, l2);
            s.mx += c0 * s.sx; s.my += c1 * s.sy; s.mz += c2 * s.sz;
            mask = (uint32_t)l0 | ((uint32_t)l1 << 1) | ((uint32_t)l2 << 2);
            it_up += (uint32_t)(c0 + c1 + c2);
            st_jump(stats, lvl);
            // every iteration steps each axis at most once: once one axis alone has taken maxSteps steps the
            // literal loop is certainly exhausted
            int klo = iabs(s.mx - mx0); int k1 = iabs(s.my - my0); int k2 = iabs(s.mz - mz0);
            klo = klo > k1 ? klo : k1; klo = klo > k2 ? klo : k2;
            if ((uint32_t)klo >= maxSteps) break;
        }
    }
    if (hit) {
        int klo = iabs(s.mx - mx0); int k1 = iabs(s.my - my0); int k2 = iabs(s.mz - mz0);
        klo = klo > k1 ? klo : k1; klo = klo > k2 ? klo : k2;
        if (it_up < maxSteps) {
            material = voxel_at(v, s.mx, s.my, s.mz);     // the literal loop reaches this fetch within its budget
        } else if ((uint32_t)klo >= maxSteps) {
            hit = false;                                  // certainly exhausted before reaching this voxel
        } else {
            st_retrace(stats);                            // ties make the count ambiguous: decide literally
            trace_literal<VRT_TRAVERSAL_BITMASK>(v, o2, start, dir, maxSteps, r);
            return;
        }
    }
    finish(s, material, mask, hit ? it_up + 1u : it_up, r);
}

// DFJ: DF with the long runs done in closed form.  A lane whose clearance is >= kJumpMin does not walk its run: the
// cube its clearance guarantees empty is exactly the kind of region trace_jump() leaves in one step, so it jumps to the
// cube's exit (or as far as its sideDist binades allow) with the integer closed form above, independently of the other
// lanes.  Lanes with small clearances walk wave-cooperative runs as in DF.  Iteration counts become bounds
// (lo <= iterations <= lo + slack); hits that straddle the budget are re-traced literally, as in JUMP.
template <class STATS>
VRT_HD void trace_dfj(const VolumeView& v, f3 start, f3 dir, uint32_t maxSteps, RayInt& r, STATS& stats)
{
    constexpr uint32_t kJumpMin = 12u;
    DdaState s;
    dda_setup(v, start, dir, s);
    uint32_t mask = s.mask, material = 0;
    bool done = false, hit = false;
    uint32_t clear = 63u;
    const uint32_t oct = (uint32_t)(s.sx > 0) | ((uint32_t)(s.sy > 0) << 1) | ((uint32_t)(s.sz > 0) << 2);
    const size_t octant = (size_t)oct * (size_t)v.df_stride;
    const float kInf = u2f(0x7F800000u);
    const float gx = s.dx < kInf ? fabsf(dir.x) : 0.0f, gy = s.dy < kInf ? fabsf(dir.y) : 0.0f, gz = s.dz < kInf ? fabsf(dir.z) : 0.0f;
    uint32_t lo = 0, slack = 0;                                // lo <= DDA iterations done so far <= lo + slack
    for (;;) {
        if (!done) {
            if (lo >= maxSteps || oob(v, s.mx, s.my, s.mz)) done = true;       // certainly out of budget, or out of the volume
            else {
                clear = v.df[octant + df_index(v, s.mx, s.my, s.mz)];
                st_lookup(stats);
                if (clear == 0u) { hit = true; done = true; }
            }
        }
        if (wave_all(done)) break;
        const bool jumper = !done && clear >= kJumpMin;
        if (jumper) {
            JumpAxis ax, ay, az;
            jump_axis_prepare(s.sdx, s.dx, s.sx, (int)clear, ax);
            jump_axis_prepare(s.sdy, s.dy, s.sy, (int)clear, ay);
            jump_axis_prepare(s.sdz, s.dz, s.sz, (int)clear, az);
            uint32_t Tstar = ax.T < ay.T ? ax.T : ay.T;
            Tstar = Tstar < az.T ? Tstar : az.T;
            if (Tstar == 0xFFFFFFFFu) { done = true; }        // direction (0,0,0): the literal loop spins to its budget -> miss
            else {
                bool l0, l1, l2;
                int c0 = jump_axis_apply(ax, Tstar, s.dx, s.sdx, l0);
                int c1 = jump_axis_apply(ay, Tstar, s.dy, s.sdy, l1);
                int c2 = jump_axis_apply(az, Tstar, s.dz, s.sdz, l2);
                s.mx += c0 * s.sx; s.my += c1 * s.sy; s.mz += c2 * s.sz;
                mask = (uint32_t)l0 | ((uint32_t)l1 << 1) | ((uint32_t)l2 << 2);
                int cm = c0 > c1 ? c0 : c1; cm = cm > c2 ? cm : c2;
                lo += (uint32_t)cm; slack += (uint32_t)(c0 + c1 + c2 - cm);
                st_jump(stats, 3);
            }
        }
        const bool walker = !done && !jumper;
        if (wave_any(walker)) {
            uint32_t kw = wave_min_u6(walker ? clear : 63u);
            st_jump(stats, 1);
            if (walker) {
                const float ox = s.sdx, oy = s.sdy, oz = s.sdz;
                for (uint32_t j = 1; j < kw; j++) {
                    uint32_t bx = f2u(s.sdx), by = f2u(s.sdy), bz = f2u(s.sdz);
                    uint32_t mn = umin3(bx, by, bz);
                    s.sdx = bx == mn ? s.sdx + s.dx : s.sdx;
                    s.sdy = by == mn ? s.sdy + s.dy : s.sdy;
                    s.sdz = bz == mn ? s.sdz + s.dz : s.sdz;
                }
                {
                    uint32_t bx = f2u(s.sdx), by = f2u(s.sdy), bz = f2u(s.sdz);
                    uint32_t mn = umin3(bx, by, bz);
                    bool k0 = bx == mn, k1 = by == mn, k2 = bz == mn;
                    mask = (uint32_t)k0 | ((uint32_t)k1 << 1) | ((uint32_t)k2 << 2);
                    s.sdx = k0 ? s.sdx + s.dx : s.sdx;
                    s.sdy = k1 ? s.sdy + s.dy : s.sdy;
                    s.sdz = k2 ? s.sdz + s.dz : s.sdz;
                }
                int nx = steps_taken((s.sdx - ox) * gx), ny = steps_taken((s.sdy - oy) * gy), nz = steps_taken((s.sdz - oz) * gz);
                s.mx += s.sx < 0 ? -nx : nx;
                s.my += s.sy < 0 ? -ny : ny;
                s.mz += s.sz < 0 ? -nz : nz;
                lo += kw;
            }
        }
    }
    if (hit) {
        if (lo + slack < maxSteps) material = voxel_at(v, s.mx, s.my, s.mz);   // the literal loop reaches this fetch within its budget
        else if (lo >= maxSteps) hit = false;                                   // certainly exhausted before it
        else {
            st_retrace(stats);
            trace_df(v, start, dir, maxSteps, r, stats);                         // ambiguous (ties near the budget): decide literally
            return;
        }
    }
    finish(s, material, mask, hit ? lo + slack + 1u : lo + slack, r);
}

} // namespace vrt
