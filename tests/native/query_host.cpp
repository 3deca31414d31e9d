// query_host.cpp -- TEST HELPER: the ray queries' per-ray code (csrc/vrt_query.h over csrc/vrt_traverse.h and the marches, csrc/vrt_march_*.h) compiled for the host,
// so that the record a query returns can be compared with the oracle's vo_trace_ray without a GPU.  The volumes are built by
// traverse_host.cpp's builders (th_create: dense fields, thb_create: bricks).  Built on demand by tests/test_ray_query_cpu.py.
#include "../../include/vrt.h"
#include "traverse_host.cpp"
#include "../../voxel-raytracing_amd/csrc/vrt_query.h"

extern "C" {

// bricks == 0: p is th_create's volume, marched with VRT_TRAVERSAL_DF; else thb_create's, with the brick march.  anyhit: only
// material is written (1 / 0).  recovered (may be NULL; closest hit, dense): 3 ints per ray -- the hit's mapPos as
// query_recover_voxel finds it from the ray's FIRST mapPos and its final sideDist (what the look-up loop's kernels report).
void qh_query(void* p, int bricks, int anyhit, int n, const float* starts, const float* dirs, uint32_t maxSteps,
              uint8_t* material, float* pos, int32_t* voxel, int8_t* normal, int32_t* recovered)
{
    const VolumeView& v = bricks ? ((HostBricks*)p)->v : ((HostVolume*)p)->v;
    for (int i = 0; i < n; i++) {
        const f3 s = mk3(starts[i * 3], starts[i * 3 + 1], starts[i * 3 + 2]);
        const f3 d = mk3(dirs[i * 3], dirs[i * 3 + 1], dirs[i * 3 + 2]);
        QueryHit h;
        if (anyhit) {
            if (bricks) query_ray<VRT_TRAVERSAL_BRICK, true>(v, s, d, maxSteps, h);
            else        query_ray<VRT_TRAVERSAL_DF, true>(v, s, d, maxSteps, h);
            material[i] = h.material != 0u ? 1 : 0;
            continue;
        }
        if (bricks) query_ray<VRT_TRAVERSAL_BRICK, false>(v, s, d, maxSteps, h);
        else        query_ray<VRT_TRAVERSAL_DF, false>(v, s, d, maxSteps, h);
        material[i] = (uint8_t)h.material;
        pos[i * 3] = h.pos.x; pos[i * 3 + 1] = h.pos.y; pos[i * 3 + 2] = h.pos.z;
        voxel[i * 3] = h.vx; voxel[i * 3 + 1] = h.vy; voxel[i * 3 + 2] = h.vz;
        normal[i * 3] = (int8_t)h.nx; normal[i * 3 + 1] = (int8_t)h.ny; normal[i * 3 + 2] = (int8_t)h.nz;
        if (recovered && !bricks) {
            RayInt r; NoStats ns;
            trace_df(v, s, d, maxSteps, r, ns);
            DdaState s0;
            dda_setup(v, s, d, s0);
            r.mx = s0.mx; r.my = s0.my; r.mz = s0.mz;                  // as trace_df_fast leaves them
            int mx = 0, my = 0, mz = 0;
            if (r.material != 0u) query_recover_voxel(r, d, mx, my, mz);
            recovered[i * 3] = mx; recovered[i * 3 + 1] = my; recovered[i * 3 + 2] = mz;
        }
    }
}

// What query_recover_voxel rounds, for the dense volume: per ray and axis x = side * g + c as the look-up loop forms it (0 for an axis
// that cannot step) and the ray's FIRST mapPos, from VRT_TRAVERSAL_DF's RayInt.  The steps the axis really took are the hit's
// mapPos minus the first one, so |x - steps| is the recovery's error (tests/test_ray_query_cpu.py prints its maximum).
void qh_recover_args(void* p, int n, const float* starts, const float* dirs, uint32_t maxSteps, float* x, int32_t* first)
{
    const VolumeView& v = ((HostVolume*)p)->v;
    const float kInf = u2f(0x7F800000u);
    for (int i = 0; i < n; i++) {
        const f3 s = mk3(starts[i * 3], starts[i * 3 + 1], starts[i * 3 + 2]);
        const f3 d = mk3(dirs[i * 3], dirs[i * 3 + 1], dirs[i * 3 + 2]);
        RayInt r; NoStats ns;
        trace_df(v, s, d, maxSteps, r, ns);
        DdaState s0;
        dda_setup(v, s, d, s0);
        x[i * 3] = s0.dx < kInf ? r.side.x * d.x + (-(s0.sdx * d.x)) : 0.0f;
        x[i * 3 + 1] = s0.dy < kInf ? r.side.y * d.y + (-(s0.sdy * d.y)) : 0.0f;
        x[i * 3 + 2] = s0.dz < kInf ? r.side.z * d.z + (-(s0.sdz * d.z)) : 0.0f;
        first[i * 3] = s0.mx; first[i * 3 + 1] = s0.my; first[i * 3 + 2] = s0.mz;
    }
}

// the ray a lane without one is given: does the march end it in iteration 0, without a look-up?
int qh_no_ray_ends_at_once(void* p, int bricks)
{
    const VolumeView& v = bricks ? ((HostBricks*)p)->v : ((HostVolume*)p)->v;
    f3 s, d;
    query_no_ray(s, d);
    DdaState st;
    dda_setup(v, s, d, st);
    return oob(v, st.mx, st.my, st.mz) ? 1 : 0;
}

size_t qh_sizeof_ray_hits() { return sizeof(vrt_ray_hits); }

// ---- shared with query_edge_main.cpp (the stand-alone program of the sanitizer run) ----
// the volume both sides trace: cell (x, y, z) of a W x H x D volume in [z][y][x] order; 1 in 200 cells solid, a slab, an empty corner
void qe_fill(uint8_t* vol, int W, int H, int D)
{
    uint32_t x = 12345u;
    for (int i = 0; i < W * H * D; i++) {
        x = x * 1664525u + 1013904223u;
        vol[i] = ((x >> 8) % 200u) == 0u ? (uint8_t)(1u + (x >> 20) % 255u) : (uint8_t)0;
    }
    for (int z = D / 2; z < D; z++)
        for (int y = 0; y < (H / 8 > 1 ? H / 8 : 1); y++)
            for (int xx = 0; xx < W; xx++) vol[xx + (y + z * H) * W] |= 7;
    for (int z = 0; z < 8; z++)
        for (int y = 0; y < 8; y++)
            for (int xx = 0; xx < 8; xx++) vol[xx + (y + z * H) * W] = 0;
}

// one budget on one scene, appended to `out` in the order query_edge_main.cpp states; returns the number of bytes written
size_t qe_records(void* scene, int bricks, int n, const float* rays, uint32_t maxSteps, uint8_t* out)
{
    std::vector<float> starts((size_t)n * 3), dirs((size_t)n * 3);
    for (int i = 0; i < n; i++)
        for (int a = 0; a < 3; a++) { starts[(size_t)i * 3 + a] = rays[(size_t)i * 6 + a]; dirs[(size_t)i * 3 + a] = rays[(size_t)i * 6 + 3 + a]; }
    std::vector<uint8_t> mat(n), any(n);
    std::vector<float> pos((size_t)n * 3);
    std::vector<int32_t> vox((size_t)n * 3), rec((size_t)n * 3);
    std::vector<int8_t> nrm((size_t)n * 3);
    qh_query(scene, bricks, 0, n, starts.data(), dirs.data(), maxSteps, mat.data(), pos.data(), vox.data(), nrm.data(), bricks ? nullptr : rec.data());
    qh_query(scene, bricks, 1, n, starts.data(), dirs.data(), maxSteps, any.data(), nullptr, nullptr, nullptr, nullptr);
    uint8_t* o = out;
    auto put = [&](const void* p, size_t bytes) { memcpy(o, p, bytes); o += bytes; };
    put(mat.data(), (size_t)n); put(pos.data(), (size_t)n * 12); put(vox.data(), (size_t)n * 12); put(nrm.data(), (size_t)n * 3);
    if (!bricks) put(rec.data(), (size_t)n * 12);
    put(any.data(), (size_t)n);
    return (size_t)(o - out);
}

} // extern "C"
