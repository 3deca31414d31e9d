// vrt_api_query.hip -- the ray queries of the C-ABI (vrt_trace_rays, vrt_occluded_rays, vrt_pick_pixels; kernel: vrt_query.hip) and
// their forms with a distance limit per ray (vrt_trace_segments, vrt_occluded_segments; kernel: vrt_query_seg.hip).
#include <cstring>

#include "vrt_host.h"

using namespace vrt;

namespace {

const int64_t kMaxQueryRays = (int64_t)1 << 28;       // k_query indexes a plane's dwords in 32 bits (3 per ray)

// the arguments all three entry points share, scalars first: nothing here touches the context or the device
int query_args(const char* who, const vrt_ctx* c, const vrt_scene* s, int64_t n, const void* in0, const void* in1, uint32_t max_steps)
{
    if (n < 0) return fail(VRT_ERR_INVALID, std::string(who) + ": n < 0");
    if (n > kMaxQueryRays) return fail(VRT_ERR_INVALID, std::string(who) + ": more than 2^28 rays in one call (the kernel indexes its planes in 32 bits; include/vrt.h)");
    if (max_steps == 0u) return fail(VRT_ERR_INVALID, std::string(who) + ": max_steps == 0");
    if (!c || !s || !in0 || !in1) return fail(VRT_ERR_INVALID, std::string(who) + ": NULL argument");
    return VRT_OK;
}

// What VRT_TRAVERSAL_AUTO resolves to for the scene, and the view the march reads: the scene's own, with the launch's
// variants as vrt_render_geometry sets them for a launch without count planes (of the context options only what
// trace_int reads from the view: "thresh_runs"; "df_prefetch", "df_own" and "open_cells" were settled when the scene was built).
int query_view(const vrt_ctx* c, const vrt_scene* s, uint32_t max_steps, VolumeView& vol)
{
    vol = s->d.vol;
    vol.count_marched = 0u; vol.count_lookups = 0u;
    if (s->bricks) {
        vol.df_thresh = (c->opt.thresh_runs && max_steps >= 32u) ? 1u : 0u;
        return VRT_TRAVERSAL_BRICK;
    }
    // the hand-written look-up loop where the ninth field exists and the budget is one its position recovery is exact for
    const bool fast = s->d.vol.df_fast != 0u && max_steps <= 1024u;
    const int W = s->d.vol.W, H = s->d.vol.H, D = s->d.vol.D;
    const int dmax = W > H ? (W > D ? W : D) : (H > D ? H : D);
    vol.df_thresh = (fast && c->opt.thresh_runs && dmax <= 1022 && max_steps >= 32u) ? 1u : 0u;
    return fast ? VRT_TRAVERSAL_DF_FAST : VRT_TRAVERSAL_DF;
}

int query_launch(vrt_ctx* c, const vrt_scene* s, QueryParams& p, int anyhit, int pick, const char* who)
{
    HIPCHK(hipSetDevice(c->device));
    const void* ptrs[7] = {p.origins, p.dirs, p.xy, p.material, p.pos, p.voxel, p.normal};
    int prc = check_device_ptrs(c, 2, ptrs, 7, who);
    if (prc != VRT_OK) return prc;
    const int trav = query_view(c, s, p.max_steps, p.vol);
    HIPCHK(launch_query(p, trav, anyhit, pick, c->stream));
    return VRT_OK;
}

// the same for a segment query; of the context options "thresh_runs" and "segment_budget" are looked at
int segment_launch(vrt_ctx* c, const vrt_scene* s, QuerySegParams& p, int anyhit, const char* who)
{
    HIPCHK(hipSetDevice(c->device));
    const void* ptrs[8] = {p.origins, p.dirs, p.t_max, p.material, p.pos, p.voxel, p.normal, p.t};
    int prc = check_device_ptrs(c, 2, ptrs, 8, who);
    if (prc != VRT_OK) return prc;
    const int trav = query_view(c, s, p.max_steps, p.vol);
    p.wave_budget = c->opt.segment_budget ? 1u : 0u;
    HIPCHK(launch_query_seg(p, trav, anyhit, c->stream));
    return VRT_OK;
}

} // namespace

extern "C" {

int vrt_trace_rays(vrt_ctx* c, const vrt_scene* s, int64_t n, const float* origins, const float* dirs, uint32_t max_steps, const vrt_ray_hits* out)
{
    int rc = query_args("vrt_trace_rays", c, s, n, origins, dirs, max_steps);
    if (rc != VRT_OK) return rc;
    if (!out) return fail(VRT_ERR_INVALID, "vrt_trace_rays: NULL argument");
    if (!out->material && !out->pos && !out->voxel && !out->normal) return fail(VRT_ERR_INVALID, "vrt_trace_rays: no output plane");
    if (n == 0) return VRT_OK;
    QueryParams p;
    memset(&p, 0, sizeof p);
    p.origins = origins; p.dirs = dirs; p.n = (uint32_t)n; p.max_steps = max_steps;
    p.material = out->material; p.pos = out->pos; p.voxel = out->voxel; p.normal = out->normal;
    return query_launch(c, s, p, 0, 0, "vrt_trace_rays");
}

int vrt_occluded_rays(vrt_ctx* c, const vrt_scene* s, int64_t n, const float* origins, const float* dirs, uint32_t max_steps, uint8_t* occluded)
{
    int rc = query_args("vrt_occluded_rays", c, s, n, origins, dirs, max_steps);
    if (rc != VRT_OK) return rc;
    if (!occluded) return fail(VRT_ERR_INVALID, "vrt_occluded_rays: no output plane");
    if (n == 0) return VRT_OK;
    QueryParams p;
    memset(&p, 0, sizeof p);
    p.origins = origins; p.dirs = dirs; p.n = (uint32_t)n; p.max_steps = max_steps;
    p.material = occluded;
    return query_launch(c, s, p, 1, 0, "vrt_occluded_rays");
}

int vrt_pick_pixels(vrt_ctx* c, const vrt_scene* s, const vrt_push* push, uint32_t max_steps, int64_t n, const int32_t* xy, const vrt_ray_hits* out)
{
    int rc = query_args("vrt_pick_pixels", c, s, n, push, xy, max_steps);
    if (rc != VRT_OK) return rc;
    if (!out) return fail(VRT_ERR_INVALID, "vrt_pick_pixels: NULL argument");
    if (!out->material && !out->pos && !out->voxel && !out->normal) return fail(VRT_ERR_INVALID, "vrt_pick_pixels: no output plane");
    const int W = push->screen_size[0], H = push->screen_size[1];
    if (W <= 0 || H <= 0 || W > 32768 || H > 32768) return fail(VRT_ERR_INVALID, "vrt_pick_pixels: bad screen_size");
    if (push->volume_bounds[0] != (uint32_t)s->d.vol.W || push->volume_bounds[1] != (uint32_t)s->d.vol.H || push->volume_bounds[2] != (uint32_t)s->d.vol.D)
        return fail(VRT_ERR_INVALID, "vrt_pick_pixels: push.volume_bounds must equal the scene dimensions (voxel_renderer.cpp:74)");
    if (n == 0) return VRT_OK;
    QueryParams p;
    memset(&p, 0, sizeof p);
    p.xy = xy; p.n = (uint32_t)n; p.max_steps = max_steps;
    p.material = out->material; p.pos = out->pos; p.voxel = out->voxel; p.normal = out->normal;
    // the pixel-independent part of ray generation, as a rendered frame's slot holds it (render_frames)
    p.rg = raygen_consts(*push);
    for (int a = 0; a < 3; a++) { p.cam_right[a] = push->cam_right[a]; p.cam_pos[a] = push->cam_pos[a]; }
    p.rcp_w = 1.0f / (float)W; p.rcp_h = 1.0f / (float)H; p.fast_screen_div = screen_div_ok(c, W, H); p.W = W; p.H = H;
    return query_launch(c, s, p, 0, 1, "vrt_pick_pixels");
}

int vrt_trace_segments(vrt_ctx* c, const vrt_scene* s, int64_t n, const float* origins, const float* dirs, const float* t_max,
                       uint32_t max_steps, const vrt_ray_hits* out, float* t_hit)
{
    int rc = query_args("vrt_trace_segments", c, s, n, origins, dirs, max_steps);
    if (rc != VRT_OK) return rc;
    if (!t_max) return fail(VRT_ERR_INVALID, "vrt_trace_segments: NULL t_max");
    if (!t_hit && (!out || (!out->material && !out->pos && !out->voxel && !out->normal))) return fail(VRT_ERR_INVALID, "vrt_trace_segments: no output plane");
    if (n == 0) return VRT_OK;
    QuerySegParams p;
    memset(&p, 0, sizeof p);
    p.origins = origins; p.dirs = dirs; p.t_max = t_max; p.n = (uint32_t)n; p.max_steps = max_steps; p.t = t_hit;
    if (out) { p.material = out->material; p.pos = out->pos; p.voxel = out->voxel; p.normal = out->normal; }
    return segment_launch(c, s, p, 0, "vrt_trace_segments");
}

int vrt_occluded_segments(vrt_ctx* c, const vrt_scene* s, int64_t n, const float* origins, const float* dirs, const float* t_max,
                          uint32_t max_steps, uint8_t* occluded)
{
    int rc = query_args("vrt_occluded_segments", c, s, n, origins, dirs, max_steps);
    if (rc != VRT_OK) return rc;
    if (!t_max) return fail(VRT_ERR_INVALID, "vrt_occluded_segments: NULL t_max");
    if (!occluded) return fail(VRT_ERR_INVALID, "vrt_occluded_segments: no output plane");
    if (n == 0) return VRT_OK;
    QuerySegParams p;
    memset(&p, 0, sizeof p);
    p.origins = origins; p.dirs = dirs; p.t_max = t_max; p.n = (uint32_t)n; p.max_steps = max_steps;
    p.material = occluded;
    return segment_launch(c, s, p, 1, "vrt_occluded_segments");
}

} // extern "C"
