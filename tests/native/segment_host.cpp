// segment_host.cpp -- TEST HELPER: the segment queries' per-ray code (csrc/vrt_query_seg.h over csrc/vrt_query.h and the marches) compiled
// for the host, so that the records, t_hit and the iteration bound can be compared with the oracle and tests/segment_reference.py
// without a GPU.  The volumes are built by traverse_host.cpp's builders (th_create: dense fields, thb_create: bricks).  Built on
// demand by tests/test_segments_cpu.py.
#include "../../include/vrt.h"
#include "traverse_host.cpp"
#include "../../voxel-raytracing_amd/csrc/vrt_query_seg.h"

extern "C" {

// bricks == 0: p is th_create's volume, marched with VRT_TRAVERSAL_DF; else thb_create's, with the brick march.  anyhit: only
// material is written (1 / 0), the occluded plane of vrt_occluded_segments.  own_budget: every ray is marched with
// min(max_steps, ceil(query_segment_bound)) as k_query_seg marches a wave whose longest segment is this ray's -- the tightest budget
// the kernel can ever give it.
void sh_segments(void* p, int bricks, int anyhit, int own_budget, int n, const float* starts, const float* dirs, const float* t_max, uint32_t budget,
                 uint8_t* material, float* pos, int32_t* voxel, int8_t* normal, float* t)
{
    const VolumeView& v = bricks ? ((HostBricks*)p)->v : ((HostVolume*)p)->v;
    for (int i = 0; i < n; i++) {
        uint32_t maxSteps = budget;
        if (own_budget) {
            const float need = query_segment_bound(v, mk3(starts[i * 3], starts[i * 3 + 1], starts[i * 3 + 2]), mk3(dirs[i * 3], dirs[i * 3 + 1], dirs[i * 3 + 2]), t_max[i]);
            if (need < (float)maxSteps) maxSteps = (uint32_t)ceilf(need);
        }
        const f3 s = mk3(starts[i * 3], starts[i * 3 + 1], starts[i * 3 + 2]);
        const f3 d = mk3(dirs[i * 3], dirs[i * 3 + 1], dirs[i * 3 + 2]);
        QueryHit h;
        float th;
        if (anyhit) {
            if (bricks) query_segment_ray<VRT_TRAVERSAL_BRICK, true>(v, s, d, t_max[i], maxSteps, h, th);
            else        query_segment_ray<VRT_TRAVERSAL_DF, true>(v, s, d, t_max[i], maxSteps, h, th);
            material[i] = h.material != 0u ? 1 : 0;
            continue;
        }
        if (bricks) query_segment_ray<VRT_TRAVERSAL_BRICK, false>(v, s, d, t_max[i], maxSteps, h, th);
        else        query_segment_ray<VRT_TRAVERSAL_DF, false>(v, s, d, t_max[i], maxSteps, h, th);
        material[i] = (uint8_t)h.material;
        pos[i * 3] = h.pos.x; pos[i * 3 + 1] = h.pos.y; pos[i * 3 + 2] = h.pos.z;
        voxel[i * 3] = h.vx; voxel[i * 3 + 1] = h.vy; voxel[i * 3 + 2] = h.vz;
        normal[i * 3] = (int8_t)h.nx; normal[i * 3 + 1] = (int8_t)h.ny; normal[i * 3 + 2] = (int8_t)h.nz;
        t[i] = th;
    }
}

// query_segment_bound of every ray
void sh_bound(void* p, int bricks, int n, const float* starts, const float* dirs, const float* t_max, float* bound)
{
    const VolumeView& v = bricks ? ((HostBricks*)p)->v : ((HostVolume*)p)->v;
    for (int i = 0; i < n; i++)
        bound[i] = query_segment_bound(v, mk3(starts[i * 3], starts[i * 3 + 1], starts[i * 3 + 2]), mk3(dirs[i * 3], dirs[i * 3 + 1], dirs[i * 3 + 2]), t_max[i]);
}

size_t sh_sizeof_ray_hits() { return sizeof(vrt_ray_hits); }

} // extern "C"
