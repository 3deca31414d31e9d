// vrt_shade.h -- the shading path of the render stage, device only: traceRay (trace_ray), skyColor, randomDir, K2's ray generation (primary_dir), the secondary
// rays of a hit (secondary_rays), color() / colorHit() (shade_eval, color_hit) and colorMainRay in its two forms
// (color_main_ray: a stack of hits; color_main_ray_packed: one word per hit).  voxel_volume.frag:80-105, :176-307.
// Used by K1, K2 and k_hit_colors (vrt_device.hip).
//
// ---- the launch contract of this code -------------------------------------------------------------------------------------
// A kernel that calls into this header owes it the following; none of it is checked here.
//
// 1. LDS.  secondary_rays<TRAV, Occ, SEC = true> traces the AO rays through a pool in LDS when TRAV is VRT_TRAVERSAL_DF_FAST,
//    _DF_FAST_CNT, _BRICK or _BRICK_CNT, VolumeView::ao_batch != 0 and ao_samples != 0.  Such a launch gives EVERY wave of the
//    workgroup VRT_AO_SLOT (3 840) bytes of LDS of its own, and PixCtx::ldsw is the byte address of the wave's slot in the LDS
//    address space, the same value in every lane of the wave: trace_ao_pool hands it to the loop through readfirstlane, while
//    the counter pointer here, ao_ray_store, brick_ao_store and brick_ao_pool use each lane's own value.  K1 and K2 put the slots at
//    the start of the dynamic segment, wave w at w * VRT_AO_SLOT (launch_primary_t / launch_shade_t size it; these
//    traversals stage no occupancy summaries there).  What a slot holds, rows of 64 dwords (256 B), one column per ray / pixel:
//      dense scenes (df_ao_pool_loop)   rows 0 - 11 the waiting rays (x y z dx dy dz gx gy gz idx0 voxoff tag), at 3 072 the
//                                       pixels' hit counters, at 3 328 (CNT) what the count planes report: 3 584 B
//      brick scenes (brick_ao_pool)     rows 0 - 12 the waiting rays, counters at 3 328 and 3 584 (CNT): all 3 840 B
//    Every other path (SEC = false, the other traversals, ao_batch == 0) never touches ldsw; k_hit_colors passes 0.
//
// 2. Lanes.  Everything here runs under the EXEC mask it is entered with and is wave-cooperative: the marches vote on run
//    lengths among the lanes that are there, and the pool hands its rays to the lanes that are there.  That is correct from
//    divergent code too (K1 MODE 2 / 4 and K2 call color_main_ray for the lanes that hit).  `active` (secondary_rays,
//    color_hit, color_main_ray) / `is_hit` (color_main_ray_packed) = false marks a lane that has no hit of its own and is
//    there to HELP: it owns no ray and its return value is not used, but where the AO rays go through the pool it takes rays
//    from it like every other lane (under VRT_FLAG_LOOKUP_COUNTS the bytes it asked for are added to its PixCtx::fetches).  Helpers only exist where the call site is wave-uniform -- K1 MODE >= 5
//    enters color_main_ray_packed with the whole wave once any lane hit, and its loop over the chain stays wave-uniform
//    (`__ballot(on)`); color_main_ray's last color_hit is reached by every lane that entered color_main_ray.
//    secondary_rays does not look at the hit itself: active = true traces from pos / normal whatever they hold (color_hit
//    passes active && material != 0).
//
// 3. Launch-uniform values.  These must be the same for every lane of a launch.  Read through readfirstlane (lane 0's value
//    serves the wave, silently): the VolumeView switches ao_batch (here), df_thresh (trace_df_fast, trace_brick), df_prefetch
//    and count_marched (trace_df_fast, trace_ao_pool), df_own in trace_df_fast; the view's df pointer, df_stride, W and H and
//    the budgets vrt_settings::max_steps and ao_steps (the loops' scalar operands).  Read as plain per-lane values that decide
//    branches meant to be wave-uniform: count_lookups everywhere, df_own in trace_int's brick branch, count_marched in the
//    brick march.
//    The hand-written loops also rely on what the host checked when it chose them: VolumeView::df_fast, 1 <= budget <= 1024.
//
// 4. The field guard.  The loops address the clearance fields from (W+2)(H+2) bytes IN FRONT of VolumeView::df (secondary_rays
//    forms the same pointer, `fld`), a finished lane reads the 0xFF byte at df + 9 * df_stride, and with df_prefetch a look-up
//    also asks for the bytes one row and one slice further along the ray, whichever way it points -- down to one slice in front of field 0 and up
//    to one slice behind the 0xFF byte.  A view handed to this code must therefore have at least one padded slice of
//    addressable bytes on both sides of its fields; the host allocates vrt_scene::df_guard = two slices, rounded up to 256 B,
//    in front and behind (vrt_host.h; set where the fields are allocated, vrt_api_scene.hip) for df and for df_counts.
//
// 5. No kernel arguments.  Nothing in this header reads the kernel-argument segment: GeomParams arrives by reference and may
//    be any object.  Code that does read the segment (kernarg_words, SlotOf<false>: vrt_frame_slot.h) stays out of here, so
//    that this path can be called from a kernel with other arguments.
// ---------------------------------------------------------------------------------------------------------------------------
#pragma once

#include "vrt_device_common.h"
#include "vrt_traverse.h"

namespace vrt {

// ---------------------------------------------------------------------------------------------
// traversal
// ---------------------------------------------------------------------------------------------

struct RayHit {            // RayHit, voxel_volume.frag:43-49
    uint32_t material;
    f3 pos, normal, dir;
    uint32_t ncode;        // which of the 26 face / edge / corner normals `normal` is: mask | (sx<0)<<3 | (sy<0)<<4 | (sz<0)<<5;
                           // 0xFFFFFFFF: none of them (the zero vector of rule A, or a masked axis the ray does not move along)
};

__device__ __forceinline__ f3 hit_normal(uint32_t mask, int sx, int sy, int sz)
{
    // normalize(-mask * rayStep) (frag:190): the vector has k = popcount(mask) components of +-1, so its length is
    // RN(sqrt(k)) and every non-zero component is +-RN(1 / RN(sqrt(k))) -- three constants instead of a square root
    // and three IEEE divisions (k = 0: the zero vector, canonical rule A).  A masked axis with rayStep = 0 (possible only
    // through rule A's initial mask) changes k's meaning; that case keeps the general form.
    const uint32_t k = __builtin_popcount(mask & 7u);
    const float c = k == 1u ? 1.0f : (k == 2u ? __uint_as_float(0x3f3504f3u) : __uint_as_float(0x3f13cd3au));
    const bool general = ((mask & 1u) && sx == 0) || ((mask & 2u) && sy == 0) || ((mask & 4u) && sz == 0);
    f3 n = mk3((mask & 1u) ? (float)(-sx) : 0.0f, (mask & 2u) ? (float)(-sy) : 0.0f, (mask & 4u) ? (float)(-sz) : 0.0f);
    if (general) return normalize3(n);
    return mk3(n.x * c, n.y * c, n.z * c);
}

// traceRay, voxel_volume.frag:176-196
// ONE_AXIS (the primary-only kernels): where every hit of the wave has a one-axis mask and its component lies in the range for
// which sqrt(RN(x * x)) == |x| (vrt_spec.h one_axis_len_ok), the hit distance is |x| -- the same bits, without the products, the
// sums and the IEEE square root; any other wave computes len3 as before
template <int TRAV, class Occ, bool AHEAD = false, bool PF = false, bool ONE_AXIS = false>
__device__ __forceinline__ void trace_ray(const DevScene& s, const Occ occ, f3 start, f3 dir,
                                          uint32_t maxSteps, RayHit& h, RayInt& r)
{
    trace_int<TRAV, decltype(occ.o2), AHEAD, false, PF>(s.vol, occ.o2, occ.o3, start, dir, maxSteps, r);
    h.material = r.material;
    h.dir = dir;
    // values first, one assignment to h afterwards: stores to h from both sides of the branch were being merged into
    // address-selected scratch stores (28 B of scratch per lane, which also slows the wave launch)
    f3 pos = mk3(0.0f, 0.0f, 0.0f), nrm = mk3(0.0f, 0.0f, 0.0f);
    uint32_t ncode = 0xFFFFFFFFu;
    if (r.material != 0) {
        nrm = hit_normal(r.mask, r.sx, r.sy, r.sz);
        const bool general = (r.mask & 7u) == 0u || ((r.mask & 1u) && r.sx == 0) || ((r.mask & 2u) && r.sy == 0) || ((r.mask & 4u) && r.sz == 0);
        if (!general) ncode = (r.mask & 7u) | ((uint32_t)(r.sx < 0) << 3) | ((uint32_t)(r.sy < 0) << 4) | ((uint32_t)(r.sz < 0) << 5);
        f3 m = mk3((r.mask & 1u) ? (r.side.x - r.delta.x) : 0.0f,
                   (r.mask & 2u) ? (r.side.y - r.delta.y) : 0.0f,
                   (r.mask & 4u) ? (r.side.z - r.delta.z) : 0.0f);
        float d;
        const float x1 = (r.mask & 1u) ? m.x : ((r.mask & 2u) ? m.y : m.z);
        if (ONE_AXIS && __ballot(!one_axis_len_ok(r.mask, x1)) == 0ull) d = fabsf(x1);     // (the lanes with a hit vote: wave-uniform)
        else {
            if (ONE_AXIS) asm volatile("" : "+v"(m.x));       // (a branch: without this the compiler computes the root for everybody and selects)
            d = len3(m);
        }
        pos = mk3(r.pos.x + d * dir.x, r.pos.y + d * dir.y, r.pos.z + d * dir.z);
    }
    h.pos = pos;
    h.normal = nrm;
    h.ncode = ncode;
}

// ---------------------------------------------------------------------------------------------
// shading helpers
// ---------------------------------------------------------------------------------------------

// pc: the push block of the pixel's frame; noise: the pixel's blue-noise texel, decoded on first use (it is the same for
// every AO sample and every bounce of the pixel)
// (kernels of VRT_TRAVERSAL_DF_FAST never fill iteration-count planes -- vrt_api.hip sends every launch that has them to the counting twins,
// VRT_TRAVERSAL_DF_FAST_CNT -- so for them `fetches` is dead and the compiler drops it: VRT_COUNTS(TRAV))
#define VRT_COUNTS(TRAV) ((TRAV) != VRT_TRAVERSAL_DF_FAST && (TRAV) != VRT_TRAVERSAL_BRICK)
struct PixCtx { int px, py; uint32_t fetches, rays; const vrt_push* pc; f3 noise;
                uint32_t ldsw; };    // ldsw: byte address of the wave's VRT_AO_SLOT bytes of LDS (df_ao_pool_loop): kernels that trace AO rays through the hand-written loop

// skyColor, voxel_volume.frag:98-105
__device__ __forceinline__ f3 sky_color(const DevScene& s, f3 d)
{
    float u = atan2_spec(d.z, d.x) * 0.1591f + 0.5f;
    float v = asin_spec(-d.y) * 0.3183f + 0.5f;
    uint32_t x = wrap_texel(u, s.sky_w), y = wrap_texel(v, s.sky_h);
    const float4 t = reinterpret_cast<const float4*>(s.sky)[(size_t)y * s.sky_w + x];
    return mk3(t.x, t.y, t.z);
}

// fragmentNoiseSeq + randomDir, voxel_volume.frag:80-95
__device__ __forceinline__ f3 random_dir(const DevScene& s, const vrt_push& pc, PixCtx& c, uint32_t num)
{
    uint32_t offset = num * 32u + pc.frame % 32u;
    const float g = 1.22074408460575947536f;
    const float a0 = 1.0f / g, a1 = 1.0f / (g * g), a2 = 1.0f / ((g * g) * g);
    {   // (the pixel's blue-noise texel is fetched anew for every sample: kept across the traces it cost four registers and, through the
        // branch around the fetch, a second copy of everything after it -- 1 350 instructions of the megakernel)
        float pxf = ((float)c.px + 0.5f) / 512.0f + 0.5f;
        float pyf = ((float)c.py + 0.5f) / 512.0f + 0.5f;
        uint32_t tx = wrap_texel(pxf, s.noise_w), ty = wrap_texel(pyf, s.noise_h);
        const uchar4 t = reinterpret_cast<const uchar4*>(s.noise)[(size_t)ty * s.noise_w + tx];
        c.noise = mk3(decode_unorm8(t.x), decode_unorm8(t.y), decode_unorm8(t.z));          // = t / 255.0f, exactly
    }
    float fo = (float)offset;
    float n0 = c.noise.x + fo * a0;
    float n1 = c.noise.y + fo * a1;
    float n2 = c.noise.z + fo * a2;
    n0 = n0 - floorf(n0); n1 = n1 - floorf(n1); n2 = n2 - floorf(n2);
    return normalize3(mk3(n0 * 2.0f - 1.0f, n1 * 2.0f - 1.0f, n2 * 2.0f - 1.0f));
}

// main() ray generation, voxel_volume.frag:312-322 (+ screen_quad.vert:18-31)
__device__ __forceinline__ f3 primary_dir(const FrameSlot& S, int px, int py)
{
    const RayGenConsts& g = S.rg;
    float sx = (((float)px + 0.5f) / g.W) * 2.0f - 1.0f;
    float sy = (((float)py + 0.5f) / g.H) * 2.0f - 1.0f;
    float vx = ((g.cd.x + sx * S.pc.cam_right[0]) + sy * g.planeV.x) + g.jx;
    float vy = ((g.cd.y + sx * S.pc.cam_right[1]) + sy * g.planeV.y) + g.jy;
    float vz = ((g.cd.z + sx * S.pc.cam_right[2]) + sy * g.planeV.z) + 0.0f;
    return normalize3(mk3(vx, vy, vz));
}

// (primary_v and primary_normalize, K1's form of the same: vrt_device_common.h -- the pick kernel of vrt_query.hip generates its rays with them too)

// calcAmbient + isShadowed + color + colorHit, voxel_volume.frag:205-264, in two halves: the secondary rays of a hit (what they
// find: how many AO rays hit something, whether the light is hidden) and the arithmetic on what they found.  color_hit is the two
// one after the other; the packed bounce chain (color_main_ray_packed) runs the first half on the way out and the second on the
// way back.
// SEC = false: the host has established ao_samples == 0 and shadows == 0 (K1 MODE 1), so neither loop is compiled in.
// active: the lane has a hit whose secondary rays are wanted.  Where the AO rays go through the wave's pool the function must be reached
// by the wave's other lanes as well (wave-uniform control flow at the call site): a lane without a hit of its own has no rays in
// the pool but takes rays from it like everybody else -- the pixels of a block's silhouette, and the few metallic pixels of a bounce,
// get the whole wave's help.  (Called from divergent code the pool simply serves the lanes that are there.)
template <int TRAV, class Occ, bool SEC = true>
__device__ __forceinline__ void secondary_rays(const GeomParams& P, const Occ occ, PixCtx& c, const f3 pos, const f3 normal, uint32_t depth,
                                               float& ambient, uint32_t& ao_hits, bool& shadowed, const bool active = true)
{
    const DevScene& s = P.sc;
    const vrt_settings& st = P.st;
    ambient = 0.0f; ao_hits = 0u;
    constexpr bool kBatch = TRAV == VRT_TRAVERSAL_DF_FAST || TRAV == VRT_TRAVERSAL_DF_FAST_CNT;
    if (!SEC || st.ao_samples == 0) {
        ambient = 1.0f;
    } else if (kBatch && __builtin_amdgcn_readfirstlane((int)s.vol.ao_batch) != 0) {
        // the hand-written loop: the AO rays of the wave's pixels from a pool in LDS that every lane draws on (df_ao_pool_loop) --
        // sample after sample each lane writes its pixel's ray into its column, and whichever lane is free traces it and reports
        // to the column's counter; which lane traces a ray changes nothing about what the ray finds
        constexpr bool kCnt = TRAV == VRT_TRAVERSAL_DF_FAST_CNT;
        const uint32_t ldsw = c.ldsw;
        const uint64_t act = __ballot(active);
        const uint32_t col = __builtin_amdgcn_mbcnt_hi((uint32_t)(act >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)act, 0u));
        __attribute__((address_space(3))) uint32_t* cnt = (__attribute__((address_space(3))) uint32_t*)(uintptr_t)(ldsw + 3072u + col * 4u);
        if (active) { cnt[0] = 0u; if (kCnt) cnt[64] = 0u; }
        // the fields as the loops address them (offsets count from one slice in front of field 0)
        const uint8_t* const fld = s.vol.df - (size_t)(s.vol.W + 2) * (size_t)(s.vol.H + 2);
        AoLane lane;
        ao_lane_rest(s.vol, lane);
        uint32_t next = 0u, looks = 0u, direct_hits = 0u, direct_fet = 0u;
        for (uint32_t i = 0; i < st.ao_samples; i++) {
            // The OWNER looks at its ray's first voxel itself -- every lane at once, where in the pool a ray's first look is a round of
            // the loop like any other: a ray in the open (the clearance covers its budget) and a ray that starts on a 0 byte are
            // decided here and never enter the pool; the others bring their first clearance with them and are marched from the round
            // they are taken up in.  The rays that will creep (clearance 1 or 2) wait in FRONT of the pool: the longest rays of a
            // sample start first, which is what the end of the AO phase waits for.
            bool store = false;
            uint32_t c0 = 0u;
            AoRay a;
            if (active) {
                f3 rd = random_dir(s, *c.pc, c, i + depth * st.ao_samples);
                f3 dir = mk3(normal.x + rd.x, normal.y + rd.y, normal.z + rd.z);
                f3 o = mk3(pos.x + dir.x * 0.01f, pos.y + dir.y * 0.01f, pos.z + dir.z * 0.01f);
                ao_ray_setup(s.vol, o, dir, a);
                c0 = fld[a.idx0];
                if (kCnt) looks += 1u;
                if (c0 == 0u) {                                // solid, border or open cell: the voxel id says which (frag:157 at iteration 0)
                    const uint32_t id = fld[a.idx0 + a.voxoff];
                    if (id != 0u) direct_hits++;
                    if (kCnt) { looks += 1u; direct_fet += id != 0u ? 1u : 0u; }
                } else if (c0 >= st.ao_steps) {                // nothing but empty voxels until the budget ends: a miss
                    if (kCnt) direct_fet += s.vol.count_marched != 0u ? 0u : st.ao_steps;
                } else store = true;
            }
            const bool creeps = store && c0 <= 2u;
            const uint64_t mc = __ballot(creeps), mo = __ballot(store && !creeps);
            const uint32_t nc = (uint32_t)__builtin_popcountll(mc);
            if (store) {
                const uint32_t slot = creeps ? __builtin_amdgcn_mbcnt_hi((uint32_t)(mc >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mc, 0u))
                                             : nc + __builtin_amdgcn_mbcnt_hi((uint32_t)(mo >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mo, 0u));
                ao_ray_store(ldsw, slot, a, col | (c0 << 8));
            }
            next = 0u;
            trace_ao_pool<kCnt>(s.vol, lane, ldsw, nc + (uint32_t)__builtin_popcountll(mo), i + 1u < st.ao_samples ? 1u : 0u, next, st.ao_steps, looks);
        }
        if (active) {
            ao_hits = cnt[0] + direct_hits;
            c.rays += st.ao_samples;
        }
        // (look-ups are counted by the lane that makes them, iterations for the pixel the ray belongs to)
        if (kCnt) c.fetches += s.vol.count_lookups != 0u ? looks : (active ? cnt[64] + direct_fet : 0u);
        // calcAmbient's sum (frag:219-222): one addition of 1 / aoSamples per ray that hit -- the value depends on their number only
        float sample_frac = 1.0f / (float)st.ao_samples;
        for (uint32_t q = 0; q < ao_hits; q++) ambient += sample_frac;
    } else if ((TRAV == VRT_TRAVERSAL_BRICK || TRAV == VRT_TRAVERSAL_BRICK_CNT) && __builtin_amdgcn_readfirstlane((int)s.vol.ao_batch) != 0) {
        // brick scenes: the same pool in the generic loop (brick_ao_pool)
        constexpr bool kCnt = TRAV == VRT_TRAVERSAL_BRICK_CNT;
        const uint32_t ldsw = c.ldsw;
        const uint64_t act = __ballot(active);
        const uint32_t col = __builtin_amdgcn_mbcnt_hi((uint32_t)(act >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)act, 0u));
        __attribute__((address_space(3))) uint32_t* cnt = (__attribute__((address_space(3))) uint32_t*)(uintptr_t)(ldsw + 3328u + col * 4u);
        if (active) { cnt[0] = 0u; if (kCnt) cnt[64] = 0u; }
        BrickAoLane lane;
        brick_ao_rest(lane);
        uint32_t next = 0u, looks = 0u, direct_hits = 0u, direct_fet = 0u;
        for (uint32_t i = 0; i < st.ao_samples; i++) {
            // (the owner looks at its ray's first voxel itself, as on dense scenes: rays in the open, rays on a 0 byte and rays that never
            // enter the volume are decided here; the rays that will creep wait in front of the pool)
            bool store = false;
            uint32_t c0 = 0u;
            DdaState rs; float gx = 0.0f, gy = 0.0f, gz = 0.0f;
            if (active) {
                f3 rd = random_dir(s, *c.pc, c, i + depth * st.ao_samples);
                f3 dir = mk3(normal.x + rd.x, normal.y + rd.y, normal.z + rd.z);
                f3 o = mk3(pos.x + dir.x * 0.01f, pos.y + dir.y * 0.01f, pos.z + dir.z * 0.01f);
                brick_ao_setup(s.vol, o, dir, rs, gx, gy, gz);
                if (!oob(s.vol, rs.mx, rs.my, rs.mz)) {          // (else: starts outside and misses the volume: leaves in iteration 0, no fetch)
                    const uint32_t oct = (uint32_t)(rs.sx > 0) | ((uint32_t)(rs.sy > 0) << 1) | ((uint32_t)(rs.sz > 0) << 2);
                    uint32_t m = 0u;
                    c0 = brick_clear(s.vol, rs.mx, rs.my, rs.mz, oct, rs.sx, rs.sy, rs.sz, m, kCnt ? &looks : nullptr);
                    if (c0 == 0u) { if (m != 0u) direct_hits++; if (kCnt) direct_fet += m != 0u ? 1u : 0u; }
                    else if (c0 >= st.ao_steps) { if (kCnt) direct_fet += s.vol.count_marched != 0u ? 0u : st.ao_steps; }
                    else store = true;
                }
            }
            const bool creeps = store && c0 <= 2u;
            const uint64_t mc = __ballot(creeps), mo = __ballot(store && !creeps);
            const uint32_t nc = (uint32_t)__builtin_popcountll(mc);
            if (store) {
                const uint32_t slot = creeps ? __builtin_amdgcn_mbcnt_hi((uint32_t)(mc >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mc, 0u))
                                             : nc + __builtin_amdgcn_mbcnt_hi((uint32_t)(mo >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mo, 0u));
                brick_ao_store(ldsw, slot, rs, gx, gy, gz, col | (c0 << 8));
            }
            next = 0u;
            brick_ao_pool<kCnt>(s.vol, lane, ldsw, nc + (uint32_t)__builtin_popcountll(mo), i + 1u < st.ao_samples, next, st.ao_steps, looks);
        }
        if (active) {
            ao_hits = cnt[0] + direct_hits;
            c.rays += st.ao_samples;
        }
        if (kCnt) c.fetches += s.vol.count_lookups != 0u ? looks : (active ? cnt[64] + direct_fet : 0u);
        float sample_frac = 1.0f / (float)st.ao_samples;
        for (uint32_t q = 0; q < ao_hits; q++) ambient += sample_frac;
    } else if (active) {
        float sample_frac = 1.0f / (float)st.ao_samples;
        for (uint32_t i = 0; i < st.ao_samples; i++) {
            f3 rd = random_dir(s, *c.pc, c, i + depth * st.ao_samples);
            f3 dir = mk3(normal.x + rd.x, normal.y + rd.y, normal.z + rd.z);
            f3 o = mk3(pos.x + dir.x * 0.01f, pos.y + dir.y * 0.01f, pos.z + dir.z * 0.01f);
            RayInt r;
            // AO rays have a 64-iteration budget: too short for jumps to pay, and budget ties would force re-traces
            // (the hand-written loop's kernels: every lane its own clearance is the batched path above; here the wave's smallest)
            trace_int<((TRAV == VRT_TRAVERSAL_JUMP || TRAV == VRT_TRAVERSAL_DFJ) ? VRT_TRAVERSAL_DF : TRAV), decltype(occ.o2), false, true, false, !kBatch>(s.vol, occ.o2, occ.o3, o, dir, st.ao_steps, r);   // (no prefetch: AO rays point every way, three gathers instead of one measured +18 %)
            if (VRT_COUNTS(TRAV)) c.fetches += r.fetches;
            c.rays++;
            if (r.material != 0) { ambient += sample_frac; ao_hits++; }
        }
    }
    shadowed = false;
    if (SEC && st.shadows && active) {
        f3 L = mk3(st.light_dir[0], st.light_dir[1], st.light_dir[2]);
        f3 o = mk3(pos.x + normal.x * 0.01f, pos.y + normal.y * 0.01f, pos.z + normal.z * 0.01f);
        RayInt r;
        trace_int<TRAV, decltype(occ.o2), false, true, true>(s.vol, occ.o2, occ.o3, o, L, st.max_steps, r);      // traceRayHit: only "did it hit" is used
        if (VRT_COUNTS(TRAV)) c.fetches += r.fetches;
        c.rays++;
        shadowed = r.material != 0;
    }
}

// color() of a hit (frag:236-248) and colorHit's division by depth + 1 (frag:258).  `sky` = skyColor(normal).
__device__ __forceinline__ f3 shade_eval(const GeomParams& P, uint32_t material, const f3 normal, const f3 sky, float ambient, bool shadowed,
                                         f3 reflection, uint32_t depth)
{
    const vrt_settings& st = P.st;
    float k = ambient * st.ambient_intensity;
    f3 amb = mk3(k * sky.x, k * sky.y, k * sky.z);
    f3 L = mk3(st.light_dir[0], st.light_dir[1], st.light_dir[2]);
    f3 diffuse = mk3(0.0f, 0.0f, 0.0f);
    if (!shadowed) {
        float diff = fmaxf(dot3(normal, L), 0.0f);
        diffuse = mk3((diff * st.light_color[0]) * st.light_intensity,
                      (diff * st.light_color[1]) * st.light_intensity,
                      (diff * st.light_color[2]) * st.light_intensity);
    }
    const vrt_material mat = P.sc.palette[material];
    float inv = (float)(depth + 1);
    f3 out;
    out.x = ((((diffuse.x + reflection.x * mat.metallic) + amb.x) * mat.diffuse[0]) * 1.0f) / inv;
    out.y = ((((diffuse.y + reflection.y * mat.metallic) + amb.y) * mat.diffuse[1]) * 1.0f) / inv;
    out.z = ((((diffuse.z + reflection.z * mat.metallic) + amb.z) * mat.diffuse[2]) * 1.0f) / inv;
    return out;
}

// active = false: the lane has nothing to shade and is here for the others' AO rays (secondary_rays); its result is not used
template <int TRAV, class Occ, bool SEC = true>
__device__ f3 color_hit(const GeomParams& P, const Occ occ, PixCtx& c, const RayHit& hit,
                        f3 reflection, uint32_t depth, const bool active = true)
{
    const DevScene& s = P.sc;
    float ambient; uint32_t ao_hits; bool shadowed;
    secondary_rays<TRAV, Occ, SEC>(P, occ, c, hit.pos, hit.normal, depth, ambient, ao_hits, shadowed, active && hit.material != 0);
    if (!active) return mk3(0.0f, 0.0f, 0.0f);
    if (hit.material == 0) return sky_color(s, hit.dir);
    // skyColor(hit.normal): the normal is one of 26 vectors, whose sky texels the scene holds in a table (computed by this very
    // function, k_sky_normals); any other normal is looked up here
    f3 sky;
    if (__ballot(hit.ncode == 0xFFFFFFFFu) == 0ull) {
        const float4 t = reinterpret_cast<const float4*>(s.sky_normals)[hit.ncode];
        sky = mk3(t.x, t.y, t.z);
    } else sky = sky_color(s, hit.normal);
    return shade_eval(P, hit.material, hit.normal, sky, ambient, shadowed, reflection, depth);
}

// colorMainRay, voxel_volume.frag:267-307
// BOUNCE = false: the host has established that no ray of the frame can bounce (max_bounces == 0, or no voxel of the scene has
// a metallic material): the loop and its stack of hits -- 352 bytes of scratch per lane, which every wave of the kernel is
// given whether it bounces or not -- are compiled out
template <int TRAV, class Occ, bool BOUNCE = true>
__device__ f3 color_main_ray(const GeomParams& P, const Occ occ, PixCtx& c, const RayHit& hit, const bool active = true)
{
    const DevScene& s = P.sc;
    const vrt_settings& st = P.st;
    f3 reflection = mk3(0.0f, 0.0f, 0.0f);
    if (BOUNCE && active && s.palette[hit.material].metallic > 0.0f && st.max_bounces > 0) {
        RayHit bounces[VRT_MAX_BOUNCES];
        RayHit last = hit;
        int last_idx = -1;
        int nb = st.max_bounces > VRT_MAX_BOUNCES ? VRT_MAX_BOUNCES : (int)st.max_bounces;
        for (int i = 0; i < nb; i++) {
            float k = 2.0f * dot3(last.normal, last.dir);
            f3 rdir = mk3(last.dir.x - k * last.normal.x, last.dir.y - k * last.normal.y, last.dir.z - k * last.normal.z);
            f3 o = mk3(last.pos.x + last.normal.x * 0.01f, last.pos.y + last.normal.y * 0.01f, last.pos.z + last.normal.z * 0.01f);
            RayHit rh; RayInt ri;
            trace_ray<TRAV, Occ, false, true>(s, occ, o, rdir, st.max_steps, rh, ri);
            if (VRT_COUNTS(TRAV)) c.fetches += ri.fetches;
            c.rays++;
            bounces[i] = rh;
            last = rh;
            if (last.material == 0 || s.palette[last.material].metallic <= 0.0f) { last_idx = i; break; }
        }
        for (int i = last_idx; i >= 0; i--) {
            f3 col = color_hit<TRAV>(P, occ, c, bounces[i], reflection, (uint32_t)i);
            reflection = mk3(reflection.x + col.x, reflection.y + col.y, reflection.z + col.z);
        }
    }
    return color_hit<TRAV>(P, occ, c, hit, reflection, 0, active);        // (wave-uniform again: the lanes without a hit help with the AO rays)
}

// colorMainRay with the bounce chain as ONE WORD per hit instead of a stack of RayHits (44 B each: 352 B of scratch per lane for
// every wave of the launch, and 0.6 GB of scratch writes per 4K frame on the Mandelbulb).  What the way back needs of a hit on the
// chain is what color() consumes: its material, which of the 27 normals it has (26 face / edge / corner vectors or the zero
// vector of rule A: every normal traceRay can produce, hit_normal), how many of its AO rays hit and whether its shadow ray did --
// 8 + 6 + 16 + 1 bits.  So the secondary rays of every hit are traced on the way OUT, where the hit is at hand, at one call
// site for the primary hit and every bounce; the way back is arithmetic on the words, in the order frag:300-303 prescribes.
// The secondary rays of a METALLIC bounce are traced before it is known whether the chain will end (frag:281-298: a chain of
// max_bounces metallic hits shades none of them, lastIdx = -1): in that one case they were traced for nothing, and their rays
// and steps are taken out of the count planes again, which then hold the reference's numbers as before.
// Entry k of the chain: k = 0 the primary hit, k = i + 1 bounce i (shaded with depth i; the primary with depth 0).
__device__ __forceinline__ uint32_t chain_pack(uint32_t material, const f3 n, uint32_t ao_hits, bool shadowed)
{
    // the normal's code from the vector itself: bit a = component a is not 0, bit 3 + a = it is positive (hit_normal's ncode: the
    // component is -rayStep); a masked axis the ray does not move along has a zero component and drops out of the mask, which is
    // the same vector hit_normal's general form returns
    const uint32_t nc = (uint32_t)(n.x != 0.0f) | ((uint32_t)(n.y != 0.0f) << 1) | ((uint32_t)(n.z != 0.0f) << 2) |
                        ((uint32_t)(n.x > 0.0f) << 3) | ((uint32_t)(n.y > 0.0f) << 4) | ((uint32_t)(n.z > 0.0f) << 5);
    return material | (nc << 8) | ((uint32_t)shadowed << 14) | (ao_hits << 16);
}
__device__ __forceinline__ f3 chain_shade(const GeomParams& P, uint32_t code, f3 reflection, uint32_t depth)
{
    const DevScene& s = P.sc;
    const uint32_t nc = (code >> 8) & 63u, hits = code >> 16;
    const f3 normal = hit_normal(nc & 7u, (nc & 8u) ? -1 : 1, (nc & 16u) ? -1 : 1, (nc & 32u) ? -1 : 1);
    f3 sky;
    if ((nc & 7u) != 0u) { const float4 t = reinterpret_cast<const float4*>(s.sky_normals)[nc]; sky = mk3(t.x, t.y, t.z); }
    else sky = sky_color(s, normal);                         // the zero normal of rule A
    // calcAmbient's sum: `hits` additions of 1 / ao_samples (frag:219-222), not a product
    float ambient = 1.0f;
    if (P.st.ao_samples != 0u) {
        const float sample_frac = 1.0f / (float)P.st.ao_samples;
        ambient = 0.0f;
        for (uint32_t q = 0; q < hits; q++) ambient += sample_frac;
    }
    return shade_eval(P, code & 0xFFu, normal, sky, ambient, ((code >> 14) & 1u) != 0u, reflection, depth);
}

// NBT: the most bounces the launch can ask for (the chain's words are registers: 2, 5 or VRT_MAX_BOUNCES + 1 of them)
template <int TRAV, class Occ, int NBT>
__device__ f3 color_main_ray_packed(const GeomParams& P, const Occ occ, PixCtx& c, const RayHit& hit, const bool is_hit = true)
{
    const DevScene& s = P.sc;
    const vrt_settings& st = P.st;
    const int nb = st.max_bounces > NBT ? NBT : (int)st.max_bounces;
    uint32_t codes[NBT + 1];
#pragma unroll
    for (int q = 0; q <= NBT; q++) codes[q] = 0u;
    f3 reflection = mk3(0.0f, 0.0f, 0.0f);
    RayHit cur = hit;
    int last = 0;                                              // the chain's last entry that is shaded: 0 = the primary hit alone
    uint32_t spec_fetches = 0u, spec_rays = 0u;
    // The loop over the chain's entries is WAVE-UNIFORM: a lane whose chain has ended (or that never had a hit) stays in it for as long
    // as some lane's chain goes on, and takes AO rays from the pool like the others (secondary_rays) -- the few metallic pixels of a
    // bounce get the whole wave's help.  Everything else a lane does here is under `on`: its own chain is still being followed.
    bool on = is_hit;
    for (int k = 0; __ballot(on) != 0ull; k++) {
        // the secondary rays of entry k (a hit: the primary, or a bounce that found something)
        float ambient; uint32_t ao_hits; bool shadowed;
        const uint32_t f0 = c.fetches, r0 = c.rays;
        secondary_rays<TRAV, Occ, true>(P, occ, c, cur.pos, cur.normal, k > 0 ? (uint32_t)(k - 1) : 0u, ambient, ao_hits, shadowed, on);
        if (on) {
            codes[k] = chain_pack(cur.material, cur.normal, ao_hits, shadowed);
            last = k;
            const bool metal = s.palette[cur.material].metallic > 0.0f;
            if (!metal) on = false;                            // (k = 0: no chain at all; k > 0: the chain ends on a hit that does not reflect)
            else {
                if (k > 0) { if (VRT_COUNTS(TRAV)) spec_fetches += c.fetches - f0; spec_rays += c.rays - r0; }    // a metallic bounce: shaded only if the chain ends
                if (k >= nb) { last = -1; on = false; }        // max_bounces metallic bounces (or max_bounces == 0): nothing on the chain is shaded
            }
        }
        if (on) {
            float d2 = 2.0f * dot3(cur.normal, cur.dir);
            f3 rdir = mk3(cur.dir.x - d2 * cur.normal.x, cur.dir.y - d2 * cur.normal.y, cur.dir.z - d2 * cur.normal.z);
            f3 o = mk3(cur.pos.x + cur.normal.x * 0.01f, cur.pos.y + cur.normal.y * 0.01f, cur.pos.z + cur.normal.z * 0.01f);
            RayHit rh; RayInt ri;
            trace_ray<TRAV, Occ, false, true>(s, occ, o, rdir, st.max_steps, rh, ri);
            if (VRT_COUNTS(TRAV)) c.fetches += ri.fetches;
            c.rays++;
            if (rh.material == 0u) {                           // the chain ends in the sky: colorHit of a miss is skyColor(dir)
                const f3 col = sky_color(s, rh.dir);
                reflection = mk3(reflection.x + col.x, reflection.y + col.y, reflection.z + col.z);
                on = false;
            } else cur = rh;
        }
    }
    if (!is_hit) return mk3(0.0f, 0.0f, 0.0f);
    if (last < 0) {
        // frag:281-303 with lastIdx = -1: the bounces' secondary rays were traced for nothing -- the reference never traces them
        if (VRT_COUNTS(TRAV)) c.fetches -= spec_fetches;
        c.rays -= spec_rays;
        last = 0;
    }
    // the way back: entry j (bounce j - 1) with the reflection gathered behind it, frag:300-303
#pragma unroll
    for (int j = NBT; j >= 1; j--) {
        if (j <= last) {
            const f3 col = chain_shade(P, codes[j], reflection, (uint32_t)(j - 1));
            reflection = mk3(reflection.x + col.x, reflection.y + col.y, reflection.z + col.z);
        }
    }
    return chain_shade(P, codes[0], reflection, 0u);
}

} // namespace vrt
