// sky_plane_host.cpp -- TEST HELPER: the rule that says when a launch uses a miss-colour plane (csrc/vrt_miss_plane.h:
// sky_plane_key, sky_plane_select over a SkyPlaneCache), compiled for the host without HIP.  Two builds, both by
// tests/test_sky_plane_cpu.py with g++: a shared library the test drives through ctypes, and -- with -DSKY_PLANE_MAIN and
// -fsanitize=address,undefined -- a stand-alone program whose main() runs a fixed script of launches over the same functions
// (256-frame launches, 5 views through 4 slots, groups beyond the slots, a disabled context) and exits 0 when every expectation
// holds.  Never linked into libvrt_hip.so.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../voxel-raytracing_amd/csrc/vrt_miss_plane.h"

using namespace vrt;

extern "C" {

int32_t sp_planes(void) { return VRT_SKY_PLANES; }
int32_t sp_min_group(void) { return VRT_SKY_PLANE_MIN_GROUP; }
int32_t sp_key_words(void) { return (int32_t)(sizeof(SkyPlaneKey) / 4); }

// the key of a frame: consts = the ten words of RayGenConsts followed by the three of cam_right, as bit patterns
void sp_key(const uint32_t consts[13], int32_t W, int32_t H, int32_t fast_div, uint64_t sky_gen, uint32_t* out)
{
    float rg[10], right[3];
    memcpy(rg, consts, 40); memcpy(right, consts + 10, 12);
    const SkyPlaneKey k = sky_plane_key(rg, right, W, H, fast_div, sky_gen);
    memcpy(out, k.w, sizeof k.w);
}

void* sp_cache_new(void) { return new SkyPlaneCache(); }
void sp_cache_free(void* c) { delete (SkyPlaneCache*)c; }
void sp_cache_clear(void* c) { ((SkyPlaneCache*)c)->clear(); }
int32_t sp_cache_held(void* c) { int32_t n = 0; for (int q = 0; q < VRT_SKY_PLANES; q++) n += ((SkyPlaneCache*)c)->valid[q] ? 1 : 0; return n; }

// one launch: keys = n keys of sp_key_words() words each; plane_of: n bytes out; build_from: VRT_SKY_PLANES words out.
// Returns the number of slots the launch's frames load from.
int32_t sp_select(void* c, int32_t enabled, int32_t eligible, int32_t n, const uint32_t* keys, int32_t min_group, uint8_t* plane_of, int32_t* build_from)
{
    std::vector<SkyPlaneKey> k((size_t)(n > 0 ? n : 0));
    for (int32_t f = 0; f < n; f++) memcpy(k[(size_t)f].w, keys + (size_t)f * (sizeof(SkyPlaneKey) / 4), sizeof(SkyPlaneKey));
    SkyPlaneChoice ch;
    sky_plane_select(*(SkyPlaneCache*)c, enabled != 0, eligible != 0, n, k.data(), min_group, ch);
    if (n > 0 && n <= VRT_SKY_PLANE_MAX_FRAMES) memcpy(plane_of, ch.plane_of, (size_t)n);
    memcpy(build_from, ch.build_from, sizeof ch.build_from);
    return ch.used_planes;
}

} // extern "C"

#ifdef SKY_PLANE_MAIN
namespace {

int g_bad = 0;
#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "sky_plane_host: line %d: %s\n", __LINE__, #cond); g_bad++; } } while (0)

SkyPlaneKey view(uint32_t v, int32_t W = 104, int32_t H = 40, uint64_t gen = 7)
{
    float rg[10], right[3];
    for (int i = 0; i < 10; i++) rg[i] = 0.25f * (float)(i + 1) + (float)v;
    for (int i = 0; i < 3; i++) right[i] = 1.0f / (float)(i + 1 + v);
    return sky_plane_key(rg, right, W, H, 1, gen);
}

} // namespace

int main()
{
    const int G = VRT_SKY_PLANE_MIN_GROUP;
    SkyPlaneCache c;
    SkyPlaneChoice ch;
    // a full table of one view: one plane, built from frame 0
    {
        std::vector<SkyPlaneKey> k(VRT_SKY_PLANE_MAX_FRAMES, view(0));
        sky_plane_select(c, true, true, (int)k.size(), k.data(), G, ch);
        EXPECT(ch.used_planes == 1 && ch.build_from[ch.plane_of[0] - 1] == 0);
        for (size_t f = 0; f < k.size(); f++) EXPECT(ch.plane_of[f] == ch.plane_of[0] && ch.plane_of[f] >= 1);
        sky_plane_select(c, true, true, (int)k.size(), k.data(), G, ch);               // again: held, nothing built
        for (int q = 0; q < VRT_SKY_PLANES; q++) EXPECT(ch.build_from[q] == -1);
        EXPECT(ch.used_planes == 1);
    }
    // 256 frames, every one a view of its own: no plane, nothing evicted
    {
        std::vector<SkyPlaneKey> k;
        for (uint32_t f = 0; f < VRT_SKY_PLANE_MAX_FRAMES; f++) k.push_back(view(100 + f));
        sky_plane_select(c, true, true, (int)k.size(), k.data(), G, ch);
        for (size_t f = 0; f < k.size(); f++) EXPECT(ch.plane_of[f] == 0);
        EXPECT(ch.used_planes == 0);
        int held = 0; for (int q = 0; q < VRT_SKY_PLANES; q++) held += c.valid[q] ? 1 : 0;
        EXPECT(held == 1);
    }
    // six groups of G frames in one launch: the first VRT_SKY_PLANES that find a slot get one, nobody takes another group's
    {
        c.clear();
        std::vector<SkyPlaneKey> k;
        for (uint32_t v = 0; v < 6; v++) for (int j = 0; j < G; j++) k.push_back(view(v));
        sky_plane_select(c, true, true, (int)k.size(), k.data(), G, ch);
        EXPECT(ch.used_planes == VRT_SKY_PLANES);
        bool seen[VRT_SKY_PLANES + 1] = {};
        for (uint32_t v = 0; v < 6; v++) {
            const uint8_t p = ch.plane_of[v * (uint32_t)G];
            for (int j = 0; j < G; j++) EXPECT(ch.plane_of[v * (uint32_t)G + (uint32_t)j] == p);
            EXPECT((v < VRT_SKY_PLANES) == (p != 0));
            if (p) { EXPECT(!seen[p]); seen[p] = true; }
        }
    }
    // five views one after the other through four slots: the view used longest ago goes
    {
        c.clear();
        for (uint32_t v = 0; v < 5; v++) {
            std::vector<SkyPlaneKey> k((size_t)G, view(v));
            sky_plane_select(c, true, true, G, k.data(), G, ch);
            EXPECT(ch.used_planes == 1 && ch.plane_of[0] != 0);
        }
        SkyPlaneKey one = view(0);                                  // view 0 went: a single frame of it finds nothing
        sky_plane_select(c, true, true, 1, &one, G, ch);
        EXPECT(ch.plane_of[0] == 0);
        one = view(4);                                              // view 4 is held: a single frame uses it
        sky_plane_select(c, true, true, 1, &one, G, ch);
        EXPECT(ch.plane_of[0] != 0 && ch.build_from[ch.plane_of[0] - 1] == -1);
    }
    // disabled, not eligible, no frames, too many frames
    {
        std::vector<SkyPlaneKey> k((size_t)(2 * G), view(4));
        sky_plane_select(c, false, true, (int)k.size(), k.data(), G, ch);
        EXPECT(ch.used_planes == 0 && ch.plane_of[0] == 0);
        sky_plane_select(c, true, false, (int)k.size(), k.data(), G, ch);
        EXPECT(ch.used_planes == 0 && ch.plane_of[0] == 0);
        sky_plane_select(c, true, true, 0, k.data(), G, ch);
        EXPECT(ch.used_planes == 0);
        sky_plane_select(c, true, true, VRT_SKY_PLANE_MAX_FRAMES + 1, k.data(), G, ch);
        EXPECT(ch.used_planes == 0);
    }
    if (g_bad) { fprintf(stderr, "sky_plane_host: %d expectation(s) failed\n", g_bad); return 1; }
    printf("sky_plane_host: ok\n");
    return 0;
}
#endif
