// query_host.cpp -- TEST HELPER: the ray queries' per-ray code (csrc/vrt_query.h over csrc/vrt_traverse.h) compiled for the host,
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

} // extern "C"
