// render_rays_host.cpp -- TEST HELPER with its own main: csrc/vrt_render_rays.h (over csrc/vrt_query.h and the marches) compiled for
// the host, so that the record and the G-buffer values vrt_render_rays makes of a primary ray can be compared with the oracle's
// main() without a GPU -- and so that the same code runs under AddressSanitizer + UBSan as a program of its own.
//
//   render_rays_host roundtrip
//       rays_pack -> rays_unpack over every material, mask and rayStep code; exit status 0 when it is the identity
//   render_rays_host <W> <H> <D> <volume> <rays> <records> <max_steps>...
//       <volume>: W * H * D bytes in [z][y][x] order; <rays>: n x 6 packed floats (origin, direction).  For every budget, first on the
//       dense fields (VRT_TRAVERSAL_DF) then on bricks (the brick march; dimensions that are multiples of 8), <records> receives n
//       records of 44 bytes: packed u32, depth f32, pos 3 x f32, normal8 u32, mask8 hit_id hit_mask u8 + 1 pad, hit_voxel 3 x i16 + 1
//       pad, and the voxel query_recover_voxel finds from the ray's first mapPos 3 x i16 + 1 pad (dense, budgets <= 1024; else the
//       hit voxel once more).
// Built and run by tests/test_render_rays_cpu.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/vrt.h"
#include "traverse_host.cpp"
#include "../../voxel-raytracing_amd/csrc/vrt_render_rays.h"

static int roundtrip()
{
    for (uint32_t material = 0; material < 256u; material++)
        for (uint32_t mask = 0; mask < 8u; mask++)
            for (int sx = -1; sx <= 1; sx++)
                for (int sy = -1; sy <= 1; sy++)
                    for (int sz = -1; sz <= 1; sz++) {
                        uint32_t m2, k2; int x2, y2, z2;
                        rays_unpack(rays_pack(material, mask, sx, sy, sz), m2, k2, x2, y2, z2);
                        if (m2 != material || k2 != mask || x2 != sx || y2 != sy || z2 != sz) {
                            fprintf(stderr, "roundtrip: %u %u %d %d %d -> %u %u %d %d %d\n", material, mask, sx, sy, sz, m2, k2, x2, y2, z2);
                            return 1;
                        }
                    }
    return 0;
}

static void put(std::vector<uint8_t>& out, const void* p, size_t bytes)
{
    const uint8_t* b = (const uint8_t*)p;
    out.insert(out.end(), b, b + bytes);
}

template <int TRAV>
static void records(const VolumeView& v, int n, const float* rays, uint32_t maxSteps, std::vector<uint8_t>& out)
{
    for (int i = 0; i < n; i++) {
        const f3 s = mk3(rays[i * 6], rays[i * 6 + 1], rays[i * 6 + 2]);
        const f3 d = mk3(rays[i * 6 + 3], rays[i * 6 + 4], rays[i * 6 + 5]);
        RayInt r; QueryHit h;
        rays_primary<TRAV>(v, s, d, maxSteps, r, h);
        RaysPixel g;
        rays_pixel(r, h, s, g);
        int16_t rec[4] = {g.vx, g.vy, g.vz, 0};
        if (TRAV == VRT_TRAVERSAL_DF && maxSteps <= 1024u && r.material != 0u) {
            // as the look-up loop leaves RayInt: the FIRST mapPos (vrt_query.h, query_recover_voxel)
            f3 df = d;
            query_flush_direction(df);
            DdaState s0;
            dda_setup(v, s, df, s0);
            RayInt r0 = r;
            r0.mx = s0.mx; r0.my = s0.my; r0.mz = s0.mz;
            int mx = 0, my = 0, mz = 0;
            query_recover_voxel(r0, df, mx, my, mz);
            rec[0] = (int16_t)mx; rec[1] = (int16_t)my; rec[2] = (int16_t)mz;
        }
        const uint8_t bytes[4] = {g.mask8, g.hit_id, g.hit_mask, 0};
        const int16_t vox[4] = {g.vx, g.vy, g.vz, 0};
        const float pos[3] = {g.pos.x, g.pos.y, g.pos.z};
        put(out, &g.packed, 4); put(out, &g.depth, 4); put(out, pos, 12); put(out, &g.normal8, 4);
        put(out, bytes, 4); put(out, vox, 8); put(out, rec, 8);
    }
}

static bool read_file(const char* path, std::vector<uint8_t>& buf)
{
    FILE* f = fopen(path, "rb");
    if (!f) { perror(path); return false; }
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    buf.resize((size_t)bytes);
    const bool ok = fread(buf.data(), 1, (size_t)bytes, f) == (size_t)bytes;
    fclose(f);
    if (!ok) fprintf(stderr, "%s: short read\n", path);
    return ok;
}

int main(int argc, char** argv)
{
    if (argc == 2 && strcmp(argv[1], "roundtrip") == 0) return roundtrip();
    if (argc < 8) { fprintf(stderr, "usage: %s roundtrip | <W> <H> <D> <volume> <rays> <records> <max_steps>...\n", argv[0]); return 2; }
    const int W = atoi(argv[1]), H = atoi(argv[2]), D = atoi(argv[3]);
    std::vector<uint8_t> vol, raw;
    if (W < 1 || H < 1 || D < 1 || !read_file(argv[4], vol) || !read_file(argv[5], raw)) return 2;
    if (vol.size() != (size_t)W * H * D || raw.size() % 24 != 0) { fprintf(stderr, "bad input sizes\n"); return 2; }
    const int n = (int)(raw.size() / 24);
    std::vector<float> rays((size_t)n * 6);
    memcpy(rays.data(), raw.data(), raw.size());
    void* dense = th_create(vol.data(), W, H, D);
    void* brick = (W % 8 == 0 && H % 8 == 0 && D % 8 == 0) ? thb_create(vol.data(), W, H, D) : nullptr;
    std::vector<uint8_t> out;
    for (int b = 7; b < argc; b++) {
        const uint32_t maxSteps = (uint32_t)strtoul(argv[b], nullptr, 10);
        records<VRT_TRAVERSAL_DF>(((HostVolume*)dense)->v, n, rays.data(), maxSteps, out);
        if (brick) records<VRT_TRAVERSAL_BRICK>(((HostBricks*)brick)->v, n, rays.data(), maxSteps, out);
    }
    FILE* g = fopen(argv[6], "wb");
    if (!g) { perror(argv[6]); return 2; }
    const bool ok = fwrite(out.data(), 1, out.size(), g) == out.size();
    fclose(g);
    th_destroy(dense);
    if (brick) thb_destroy(brick);
    return ok ? 0 : 2;
}
