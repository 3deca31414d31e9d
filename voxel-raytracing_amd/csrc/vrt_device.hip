// vrt_device.hip -- the render stage: hand-written HIP kernels for gfx950 (MI355X, CDNA4; 64-wide wavefronts).
//
//   k_primary<...>    K1: per-pixel ray generation + Amanatides-Woo DDA + G-buffer write
//                     (voxel_volume.frag:309-346, :109-196 of the reference)
//   k_shade<...>      K2: AO / shadow / mirror-bounce rays + shading (voxel_volume.frag:205-307)
//   k_sky_*, k_hit_colors, k_tile_tags   the tables and tags K1 reads
// (scene build: vrt_scene_build.hip; scene edits: vrt_scene_edit.hip; K3: vrt_denoise.hip; strips, blit, accumulate, resolve:
// vrt_post.hip.)  Compiled in four parts, -DVRT_K1_PART=0..3: the list behind launch_shade_t.
//
// A wave owns an 8x8 pixel block so that its 64 rays stay spatially coherent; the default (clearance-field)
// traversal runs one wave per workgroup, the LDS-staged ones 16x16 tiles of four waves.  Rays are generated in-kernel
// from the 96-byte push-constant block (no ray buffers); a launch covers up to 8 frames.  No MFMA: nothing here is a
// dense contraction.
//
// All arithmetic follows vrt_spec.h (fp32, -ffp-contract=off); the DDA state (sideDist, mapPos, mask)
// is advanced with exactly the additions of voxel_volume.frag:164-170 in every traversal mode, so hit
// voxel, mask, t and step budget are independent of the mode.
#include "vrt_device_common.h"

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

// Occupancy summaries as seen by a workgroup: LDS copies when they fit (typed address_space(3) pointers, so
// that the lookups compile to ds_read_b64 and not to flat loads), the L2-resident originals otherwise.
typedef const __attribute__((address_space(3))) uint64_t* lds_u64_ptr;
template <bool LDS> struct OccT;
template <> struct OccT<true>  { lds_u64_ptr o2, o3; };
template <> struct OccT<false> { const uint64_t* o2; const uint64_t* o3; };

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
template <int TRAV, class Occ, bool AHEAD = false, bool PF = false>
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
        float d = len3(m);
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
#if defined(VRT_NO_SKY_TABLE)
    if (false) {
#else
    if (__ballot(hit.ncode == 0xFFFFFFFFu) == 0ull) {
#endif
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

// ---------------------------------------------------------------------------------------------
// K1: primary rays
// ---------------------------------------------------------------------------------------------

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

// MODE 0: write hit records for K2 (split);  1: no secondary rays enabled, shade inline;  4: the megakernel without its bounce loop;
// MODE 5, 6, 7: the megakernel with the bounce chain as one word per hit (color_main_ray_packed: no stack of hits; what the product
//         traversals launch) for at most 2 / 5 / VRT_MAX_BOUNCES bounces;
// MODE 2: megakernel -- the lanes that hit go on to trace their AO / shadow / bounce rays in this same kernel, so that
//         the secondary rays' latency hides under the primary work of the other waves (a separate K2 launch has a
//         single round of waves and is bound by the longest ray's dependency chain).
#ifndef VRT_CHAIN_WAVES
#define VRT_CHAIN_WAVES 7     // (development: the packed-chain megakernels at 6 or 5 waves per SIMD, i.e. 80 / 96 VGPRs)
#endif
#ifndef VRT_MODE4_WAVES
#define VRT_MODE4_WAVES 7     // (development: 8 forces the megakernel without its bounce loop into 64 VGPRs, at the price of 12 B of scratch per lane)
#endif
template <int TRAV, bool OCC_LDS, int MODE, bool TABLE, int MAP>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(((MODE == 4 && TRAV == VRT_TRAVERSAL_DF_FAST) ? VRT_MODE4_WAVES : (MODE >= 5 ? VRT_CHAIN_WAVES : 7)), 8))) void k_primary(const GeomParams P)
{
    extern __shared__ __attribute__((aligned(16))) uint64_t lds_occ[];
    // the tile map arrives with one 64-byte scalar load (and one wait) before anything depends on it
    TileMap M = P.map;
#ifdef VRT_EXP_STAMPS
    const uint64_t t_begin = wall_clock64();                                 // (development build, tools/exp_timeline2.py: every wave's start / end stamp goes to the motion plane)
#else
    const uint64_t t_begin = (M.flags & 2u) ? wall_clock64() : 0ull;         // diagnostic timeline (100 MHz)
#endif
    int x0, y0, yp0, ty, tx;
    uint32_t frame;
    if (!block_to_tile<MAP>(M, frame, ty, tx)) return;                   // uniform per workgroup
    // the block's tile tag (k_tile_tags) and the frame's "the tags say nothing" word: two scalar loads that leave together with
    // the frame slot's (their address needs nothing from the slot: tags are laid out in the launch's LOCAL rows of 8x8 blocks,
    // in dispatch order), looked at after ray generation.  Written by the kernel before this one: constant address space.
    // (A launch without tags points at one word per frame that holds its tile_gen, with tags_x = 0 and tags_per_frame = 1.)
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t tile_gen = P.tile_gen;
    // (vrt_span.h: with them leave the four tags of the block's 32x8 span -- neighbours in one tag row; the block's own four times
    // over where the span is cut by the frame's right edge or the launch has no span path, the frame's one word without tags)
    uint32_t tag, tag_all, st0, st1, st2, st3;
    bool span_w;
    {
        const_u32_ptr tg = (const_u32_ptr)(P.tile_tags + (size_t)frame * P.tags_per_frame);
        const uint32_t tags_x = P.tags_x, sh = (uint32_t)M.tile >> 4;
        const uint32_t row8 = ((uint32_t)ty << sh) + (uint32_t)(wave >> 1), col8 = ((uint32_t)tx << sh) + (uint32_t)(wave & 1);
        span_w = (M.flags & VRT_MAPFLAG_SKY_SPAN) != 0u && span_in_frame(span_x0(col8), (uint32_t)M.W);
        const uint32_t own = row8 * tags_x + (tags_x ? col8 : 0u);
        const uint32_t first = (span_w && tags_x) ? own - span_role(col8) : own, step = (span_w && tags_x) ? 1u : 0u;
        st0 = tg[first]; st1 = tg[first + step]; st2 = tg[first + 2u * step]; st3 = tg[first + 3u * step];
        const uint32_t k = own - first;                           // (the block's own is one of the four)
        tag = k == 0u ? st0 : (k == 1u ? st1 : (k == 2u ? st2 : st3));
        tag_all = tg[P.tags_per_frame - 1u];
    }
    // ... and so does the frame's part of ray generation (camera, hoisted constants, strip assignment), in one batch
    RayGenConsts g;
    float cam_right[3];
    int shard_rank;
    uint32_t box;
    SlotOf<TABLE>::head(P, frame, g, cam_right, shard_rank, box);
    asm volatile("" : "+s"(box));
    // (one scalar from here on, not three: past 80 scalar registers a SIMD holds 7 of these waves, not 8)
    // (bit 0: the block has no tag; bit 1: its span may take the span path; bit 2: none of the span's blocks has a tag)
    const uint32_t untagged = (uint32_t)__builtin_amdgcn_readfirstlane(((tag != tile_gen && tag_all != tile_gen) ? 1 : 0) | (span_w ? 2 : 0) |
                                                                       (span_untagged(st0, st1, st2, st3, tag_all, tile_gen) ? 4 : 0));
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
    const bool span = (untagged & 2u) != 0u && block_skips(box, (uint32_t)px0 & ~31u, (uint32_t)py0, (untagged & 4u) != 0u);
    int px, py;
    span_pixel(span, span ? (uint32_t)px0 & ~31u : (uint32_t)px0, (uint32_t)py0, span_role((uint32_t)px0 >> 3), (uint32_t)lane, px, py);
    int W = M.W, H = M.H;
    if (px >= W || py >= H) return;
    // (two vector registers from here on, whatever they were made from: without this the megakernels' register allocation
    // changes with the choice above and the bounce chain spills one register more)
    asm volatile("" : "+v"(px), "+v"(py));
    size_t i = (size_t)py * (size_t)W + (size_t)px;

    const DevScene& s = P.sc;
    f3 start = mk3(0.0f, 0.0f, 0.0f);
    const f3 v = primary_v(g, crx, cry, crz, rcp_w, rcp_h, fast_div, px, py);
    RayHit h; RayInt r;
    // a wave whose 8x8 pixels lie outside the frame's box rectangle (FrameSlot::box, vrt_internal.h box_rect) cannot meet the
    // volume: it writes what a miss writes without testing the box (wave-uniform: the rectangle is in units of 32 pixels) --
    // and inside the rectangle neither can a wave whose block no occupied 4^3 cell of the volume projects onto (k_tile_tags)
    const bool skip = box != 0xFF00FF00u && ((uint32_t)(px0 >> 5) < boxr.x || (uint32_t)(px0 >> 5) >= boxr.y || (uint32_t)(py0 >> 5) < boxr.z ||
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
#ifndef VRT_EXP_STAMPS
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
#endif
            if (f.position) *gptr<vrt_f4>(f.position, i32 << 4) = (vrt_f4){0.0f, 0.0f, 0.0f, 0.0f};
#ifdef VRT_EXP_STAMPS
            if (f.motion) *gptr<vrt_f2>(f.motion, i32 << 3) = (vrt_f2){__uint_as_float((uint32_t)t_begin), __uint_as_float((uint32_t)wall_clock64())};
#else
            if (f.motion) *gptr<vrt_f2>(f.motion, i32 << 3) = (vrt_f2){0.0f, 0.0f};
#endif
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
        trace_ray<TRAV, OccT<kLds>, MODE == 1>(s, occ, start, dir, P.st.max_steps, h, r);   // look-ahead request: primary-only kernel
    }
    bool hit = h.material != 0;

    const vrt_frame f = SlotOf<TABLE>::planes(P, frame);   // by value: the fourteen plane pointers arrive with two scalar loads, not one by one before each store
    float depth = 0.0f;
    if (hit) depth = len3(mk3(h.pos.x - start.x, h.pos.y - start.y, h.pos.z - start.z));
    // (the reference's targets through 32-bit byte offsets from pointers SAID to be global memory -- the table form assembles
    // them from words and would otherwise get flat instructions with a 64-bit address each; the host admits frames below
    // 2^28 pixels)
    const uint32_t i32 = (uint32_t)i;
#ifndef VRT_EXP_STAMPS
    // (the launch's flags once more from the kernel's own arguments: a scalar register held across the march would be the 77th)
    const bool six = (kernarg_words(offsetof(GeomParams, map) + offsetof(TileMap, flags))[0] & VRT_MAPFLAG_SIX) != 0u;
#else
    const bool six = false;
#endif
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
#ifndef VRT_EXP_STAMPS
    if (f.motion) *gptr<vrt_f2>(f.motion, i32 << 3) = (vrt_f2){0.0f, 0.0f};
#endif
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
#ifdef VRT_EXP_LATE_INDEX
        {   // the pixel's indices once more, from px and py alone: nothing but those two stays live across the secondary rays
            int pxl = px, pyl = py;
            asm volatile("" : "+v"(pxl), "+v"(pyl));
            const size_t il = (size_t)pyl * (size_t)W + (size_t)pxl;
            store_color(f, col, il, (uint32_t)il, ((uint32_t)(yp0 + (pyl - y0)) * (uint32_t)W + (uint32_t)pxl) << 2);
        }
#else
        store_color(f, col, i, i32, ((uint32_t)(yp0 + (py - y0)) * (uint32_t)W + (uint32_t)px) << 2);
#endif
#ifdef VRT_EXP_STAMPS
        if (f.motion) *gptr<vrt_f2>(f.motion, i32 << 3) = (vrt_f2){__uint_as_float((uint32_t)t_begin), __uint_as_float((uint32_t)wall_clock64())};
#endif
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
    if (p.fused_shade == 1) launch_k1_map<TRAV, OCC_LDS, 1, TABLE>(p, grid, block, lds, s);
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
    // (the hand-written loop's AO batches: one slot of waiting rays per wave, df_ao_batch_loop)
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
