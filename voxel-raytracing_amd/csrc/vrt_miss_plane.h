// vrt_miss_plane.h -- the miss-colour plane of a view: WHEN a launch uses one.  Host only, no HIP: tests/native/sky_plane_host.cpp
// compiles this header alone (tests/test_sky_plane_cpu.py), vrt_api.hip is its one user in the library.
//
// What a miss leaves in the colour target does not depend on where the ray left from: a sky pixel's word is
// unorm8(sky_color(primary_normalize(primary_v(g, right, ..., px, py)))), a function of the frame's ray-generation constants, the
// screen size and the scene's sky -- not of the camera's position.  Frames that agree in all of those BIT FOR BIT (a dolly, a track,
// a fixed camera over an edited scene, the ranks of a sharded batch) have the same word in every sky pixel.  k_miss_plane
// (vrt_device.hip) computes the W x H words once, by K1's own long miss path, and the sky waves of the primary-only kernels of
// table launches load their pixel's word instead of generating a ray and deciding a texel (k_primary, the skip branch).
//
// The rule, stated here once:
//   * only primary-only table launches (more than VRT_MAX_BATCH frames, fused_shade == 1: the launches that run k_block_verdicts)
//     whose sky waves take the short path (GeomParams::sky_fast: the reference's targets, no diagnostic plane) are eligible, and
//     only while the context option sky_plane is on;
//   * the frames of a launch are grouped by key (SkyPlaneKey: the bytes k_miss_plane reads; compared bitwise, never with a tolerance);
//   * a group whose plane the context still holds uses it; a group of at least VRT_SKY_PLANE_MIN_GROUP frames has one built, in the
//     slot used longest ago that no group of THIS launch uses; every other frame runs the path without a plane, unchanged;
//   * the context holds at most VRT_SKY_PLANES planes.
#pragma once

#include <stdint.h>
#include <string.h>

namespace vrt {

#define VRT_SKY_PLANES 4            // planes a context keeps (the verdict byte has three bits for "which": 0 = none)
// Frames a group needs before a plane is built for it: twice the break-even of k_miss_plane's time against what a frame's sky waves
// save (profiles/sky_plane_times.json)
#define VRT_SKY_PLANE_MIN_GROUP 4
#define VRT_SKY_PLANE_MAX_FRAMES 256   // = VRT_MAX_TABLE (vrt_internal.h; vrt_api.hip asserts it)

// Everything k_miss_plane reads, as words: RayGenConsts (cd, planeV, jx, jy, W, H as floats: 10), cam_right (3), the screen size
// as the tile map holds it (2), fast_screen_div (1), and the scene's shading generation (2: unique over all scenes of the process
// and bumped whenever a sky is set -- identity and generation in one).  rcp_w and rcp_h are functions of W and H.
struct SkyPlaneKey { uint32_t w[18]; };

inline SkyPlaneKey sky_plane_key(const float rg[10], const float cam_right[3], int32_t W, int32_t H, int32_t fast_screen_div, uint64_t sky_gen)
{
    SkyPlaneKey k;
    memcpy(&k.w[0], rg, 40);
    memcpy(&k.w[10], cam_right, 12);
    k.w[13] = (uint32_t)W; k.w[14] = (uint32_t)H; k.w[15] = (uint32_t)fast_screen_div;
    k.w[16] = (uint32_t)sky_gen; k.w[17] = (uint32_t)(sky_gen >> 32);
    return k;
}
inline bool sky_plane_same(const SkyPlaneKey& a, const SkyPlaneKey& b) { return memcmp(a.w, b.w, sizeof a.w) == 0; }

// the keys of the planes a context holds and when each was last used (the device memory is the context's business)
struct SkyPlaneCache {
    SkyPlaneKey key[VRT_SKY_PLANES];
    bool        valid[VRT_SKY_PLANES] = {false, false, false, false};
    uint64_t    used[VRT_SKY_PLANES] = {0, 0, 0, 0};
    uint64_t    clock = 0;
    void clear() { for (int q = 0; q < VRT_SKY_PLANES; q++) { valid[q] = false; used[q] = 0; } }
};

// What a launch does: frame f loads from slot plane_of[f] - 1 (0: no plane), and slot q is first filled from frame build_from[q]'s
// constants (-1: it holds its plane already, or the launch does not use it).
struct SkyPlaneChoice {
    uint8_t plane_of[VRT_SKY_PLANE_MAX_FRAMES];
    int32_t build_from[VRT_SKY_PLANES];
    int32_t used_planes;                                 // slots some frame of the launch loads from
};

// The rule.  enabled: the context option; eligible: the launch is a primary-only table launch whose sky waves take the short path.
// On return the cache holds the keys of the slots to be built: the caller builds them ahead of the launch (or calls clear()).
inline void sky_plane_select(SkyPlaneCache& c, bool enabled, bool eligible, int n, const SkyPlaneKey* keys, int min_group, SkyPlaneChoice& out)
{
    memset(out.plane_of, 0, sizeof out.plane_of);
    for (int q = 0; q < VRT_SKY_PLANES; q++) out.build_from[q] = -1;
    out.used_planes = 0;
    if (!enabled || !eligible || n <= 0 || n > VRT_SKY_PLANE_MAX_FRAMES) return;
    // groups by bitwise key, in order of first appearance: first[g] = the group's first frame, group_of[f] = its group
    int first[VRT_SKY_PLANE_MAX_FRAMES], count[VRT_SKY_PLANE_MAX_FRAMES], n_groups = 0;
    int16_t group_of[VRT_SKY_PLANE_MAX_FRAMES];
    for (int f = 0; f < n; f++) {
        int g = 0;
        while (g < n_groups && !sky_plane_same(keys[first[g]], keys[f])) g++;
        if (g == n_groups) { first[g] = f; count[g] = 0; n_groups++; }
        count[g]++; group_of[f] = (int16_t)g;
    }
    int slot_of[VRT_SKY_PLANE_MAX_FRAMES];
    bool pinned[VRT_SKY_PLANES] = {false, false, false, false};
    // planes the context holds: used whatever the group's size, and safe from this launch's evictions
    for (int g = 0; g < n_groups; g++) {
        slot_of[g] = -1;
        for (int q = 0; q < VRT_SKY_PLANES; q++)
            if (c.valid[q] && sky_plane_same(c.key[q], keys[first[g]])) { slot_of[g] = q; pinned[q] = true; c.used[q] = ++c.clock; break; }
    }
    // new planes for the groups that are large enough: an empty slot, else the one used longest ago
    for (int g = 0; g < n_groups; g++) {
        if (slot_of[g] >= 0 || count[g] < min_group) continue;
        int q = -1;
        for (int j = 0; j < VRT_SKY_PLANES; j++) {
            if (pinned[j]) continue;
            if (q < 0 || (!c.valid[j] && c.valid[q]) || (c.valid[j] == c.valid[q] && c.used[j] < c.used[q])) q = j;
        }
        if (q < 0) continue;                             // (every slot serves a group of this launch already)
        c.key[q] = keys[first[g]]; c.valid[q] = true; c.used[q] = ++c.clock; pinned[q] = true;
        slot_of[g] = q; out.build_from[q] = first[g];
    }
    for (int f = 0; f < n; f++) out.plane_of[f] = (uint8_t)(slot_of[group_of[f]] + 1);
    for (int q = 0; q < VRT_SKY_PLANES; q++) out.used_planes += pinned[q] ? 1 : 0;
}

} // namespace vrt
