// vrt_api.hip -- the C-ABI of libvrt_hip.so (include/vrt.h): the error string, contexts and their options, device memory, the
// host-only calls (settings defaults, images, .vox flattening, jitter), the geometry stage (vrt_render_rays included) and the instrumentation.  Scenes are in
// vrt_api_scene.hip, their edits in vrt_api_edit.hip, the denoiser / strip packing / presentation / reprojection in vrt_api_post.hip, the ray queries in
// vrt_api_query.hip, ray generation in vrt_api_rays.hip, RCCL in vrt_api_comm.hip; vrt_host.h is what they share.  Host code only; kernels live in the other .hip files.
//
// Call surface mirrored from the reference (paths relative to its root):
//   GeometryStage::record      source/voxels/stages/geometry_stage.cpp:106-153
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "image_io.h"
#include "vox_reader.h"
#include "vrt_host.h"

using namespace vrt;

static thread_local std::string g_err;

int vrt::fail(int code, const std::string& msg) { g_err = msg; return code; }

struct OptName { const char* name; const char* env; int DevOptions::*field; };
static const OptName kOptNames[] = {
    {"tile_tags", "VRT_TILE_TAGS", &DevOptions::tile_tags}, {"box_rect", "VRT_BOX_RECT", &DevOptions::box_rect},
    {"xcd_regions", "VRT_XCD_REGIONS", &DevOptions::xcd_regions}, {"fast_loop", "VRT_FAST_LOOP", &DevOptions::fast_loop},
    {"no_bounce_kernel", "VRT_NO_BOUNCE_KERNEL", &DevOptions::no_bounce_kernel}, {"sky_fast", "VRT_SKY_FAST", &DevOptions::sky_fast},
    {"sky_span", "VRT_SKY_SPAN", &DevOptions::sky_span}, {"sky_plane", "VRT_SKY_PLANE", &DevOptions::sky_plane},
    {"packed_bounces", "VRT_PACKED_BOUNCES", &DevOptions::packed_bounces}, {"ao_batch", "VRT_AO_BATCH", &DevOptions::ao_batch}, {"tags_async", "VRT_TAGS_ASYNC", &DevOptions::tags_async},
    {"hit_table", "VRT_HIT_TABLE", &DevOptions::hit_table},
    {"thresh_runs", "VRT_THRESH_RUNS", &DevOptions::thresh_runs}, {"segment_budget", "VRT_SEGMENT_BUDGET", &DevOptions::segment_budget}, {"denoise_th16", "VRT_DENOISE_TH", &DevOptions::denoise_th16}, {"denoise_packed", "VRT_DENOISE_PACKED", &DevOptions::denoise_packed},
    {"denoise_pair", "VRT_DENOISE_PAIR", &DevOptions::denoise_pair}, {"denoise_p0", "VRT_DENOISE_P0", &DevOptions::denoise_p0}, {"denoise_pair_wgs", "VRT_DENOISE_PAIR_WGS", &DevOptions::denoise_pair_wgs},
    {"denoise_verified", "VRT_DENOISE_VERIFIED", &DevOptions::denoise_verified}, {"denoise_guard_div8", "VRT_DENOISE_GUARD_DIV8", &DevOptions::denoise_guard_div8},
    {"denoise_count", "VRT_DENOISE_COUNT", &DevOptions::denoise_count},
    {"open_cells", "VRT_OPEN_CELLS", &DevOptions::open_cells}, {"df_prefetch", "VRT_DF_PREFETCH", &DevOptions::df_prefetch},
    {"df_own", "VRT_DF_OWN", &DevOptions::df_own},
};

extern "C" {

const char* vrt_last_error(void) { return g_err.c_str(); }

int vrt_ctx_create(int device, vrt_ctx** out)
{
    if (!out) return fail(VRT_ERR_INVALID, "vrt_ctx_create: out is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(VRT_ERR_NO_DEVICE, std::string("no HIP device available (") + hipGetErrorString(e) +
                                           "); this library has no CPU fallback");
    if (device < 0 || device >= n) return fail(VRT_ERR_INVALID, "vrt_ctx_create: device index out of range");
    HIPCHK(hipSetDevice(device));
    vrt_ctx* c = new vrt_ctx();
    c->device = device;
    for (const OptName& o : kOptNames) {                       // the one place the environment is read
        const char* e = getenv(o.env);
        if (e && e[0] >= '0' && e[0] <= '9') c->opt.*(o.field) = atoi(e);        // (switches: 0 / 1; a few take small numbers)
    }
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; return fail(VRT_ERR_HIP, "hipStreamCreate failed"); }
    hipEventCreate(&c->ev_geo0); hipEventCreate(&c->ev_prim1); hipEventCreate(&c->ev_geo1);
    hipEventCreate(&c->ev_den0); hipEventCreate(&c->ev_den1);
    *out = c;
    return VRT_OK;
}

void vrt_ctx_destroy(vrt_ctx* c)
{
    if (!c) return;
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);
    if (c->tag_stream) { hipStreamSynchronize(c->tag_stream); hipStreamDestroy(c->tag_stream); }
    for (int b = 0; b < 2; b++) {
        if (c->tag_done[b]) hipEventDestroy(c->tag_done[b]);
        if (c->tag_read[b]) hipEventDestroy(c->tag_read[b]);
    }
    if (c->upload_stream) { hipStreamSynchronize(c->upload_stream); hipStreamDestroy(c->upload_stream); }
    for (int i = 0; i < vrt_ctx::kTabRing; i++) {
        if (c->tab_host[i]) hipHostFree(c->tab_host[i]);
        if (c->tab_uploaded[i]) hipEventDestroy(c->tab_uploaded[i]);
        if (c->tab_consumed[i]) hipEventDestroy(c->tab_consumed[i]);
    }
    if (c->pano_host) hipHostFree(c->pano_host);
    if (c->pano_done) hipEventDestroy(c->pano_done);
    hipEventDestroy(c->ev_geo0); hipEventDestroy(c->ev_prim1); hipEventDestroy(c->ev_geo1);
    hipEventDestroy(c->ev_den0); hipEventDestroy(c->ev_den1);
    if (c->own_stream && c->stream) hipStreamDestroy(c->stream);
    delete c;                                                  // (frees the device buffers)
}

int vrt_ctx_set_stream(vrt_ctx* c, void* hip_stream)
{
    if (!c) return fail(VRT_ERR_INVALID, "ctx is NULL");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (c->own_stream && c->stream) hipStreamDestroy(c->stream);
    c->stream = (hipStream_t)hip_stream;      // NULL is a valid handle: the HIP null (legacy default) stream
    c->own_stream = false;
    c->have_geo = c->have_den = false;
    c->checked_ptrs[0] = c->checked_ptrs[1] = c->checked_ptrs[3] = c->checked_ptrs[4] = 0;
    return VRT_OK;
}

int vrt_ctx_synchronize(vrt_ctx* c)
{
    if (!c) return fail(VRT_ERR_INVALID, "ctx is NULL");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    return VRT_OK;
}

int vrt_ctx_set_option(vrt_ctx* c, const char* name, int32_t value)
{
    if (!c || !name) return fail(VRT_ERR_INVALID, "vrt_ctx_set_option: NULL argument");
    for (const OptName& o : kOptNames)
        if (strcmp(o.name, name) == 0) { c->opt.*(o.field) = value < 0 ? 0 : value; return VRT_OK; }
    return fail(VRT_ERR_INVALID, std::string("vrt_ctx_set_option: unknown option '") + name + "'");
}

int vrt_ctx_get_option(vrt_ctx* c, const char* name, int32_t* value)
{
    if (!c || !name || !value) return fail(VRT_ERR_INVALID, "vrt_ctx_get_option: NULL argument");
    for (const OptName& o : kOptNames)
        if (strcmp(o.name, name) == 0) { *value = c->opt.*(o.field); return VRT_OK; }
    // read-only state of the miss-colour planes (vrt_miss_plane.h), for the tests: planes computed so far, planes held, the rule's
    // minimum group, and "sky_plane_of_<f>": the plane frame f of the latest launch loaded from (1 .. 4; 0: none)
    if (strcmp(name, "sky_planes_built") == 0) { *value = (int32_t)c->sky_planes_built; return VRT_OK; }
    if (strcmp(name, "sky_planes_held") == 0) { *value = 0; for (int q = 0; q < VRT_SKY_PLANES; q++) *value += c->sky_planes.valid[q] ? 1 : 0; return VRT_OK; }
    if (strcmp(name, "sky_plane_min_group") == 0) { *value = VRT_SKY_PLANE_MIN_GROUP; return VRT_OK; }
    if (strncmp(name, "sky_plane_of_", 13) == 0 && name[13] >= '0' && name[13] <= '9') {
        const int f = atoi(name + 13);
        if (f < VRT_MAX_TABLE) { *value = c->sky_plane_last[f]; return VRT_OK; }
    }
    return fail(VRT_ERR_INVALID, std::string("vrt_ctx_get_option: unknown option '") + name + "'");
}

int vrt_ctx_set_timing(vrt_ctx* c, int enabled)
{
    if (!c) return fail(VRT_ERR_INVALID, "ctx is NULL");
    c->timing = enabled != 0;
    return VRT_OK;
}

int vrt_device_info(vrt_ctx* c, char* name, size_t name_len, int* compute_units)
{
    if (!c) return fail(VRT_ERR_INVALID, "ctx is NULL");
    hipDeviceProp_t p;
    HIPCHK(hipGetDeviceProperties(&p, c->device));
    if (name && name_len) snprintf(name, name_len, "%s (%s)", p.name, p.gcnArchName);
    if (compute_units) *compute_units = p.multiProcessorCount;
    return VRT_OK;
}

int vrt_device_alloc(vrt_ctx* c, size_t bytes, void** out)
{
    if (!c || !out) return fail(VRT_ERR_INVALID, "vrt_device_alloc: NULL argument");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMalloc(out, bytes ? bytes : 1));
    return VRT_OK;
}

int vrt_device_free(vrt_ctx* c, void* p)
{
    if (!c) return fail(VRT_ERR_INVALID, "ctx is NULL");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (p) HIPCHK(hipFree(p));
    c->checked_ptrs[0] = c->checked_ptrs[1] = c->checked_ptrs[3] = c->checked_ptrs[4] = 0;     // a freed address may come back as something else: verify again
    return VRT_OK;
}

int vrt_memcpy_h2d(vrt_ctx* c, void* dst, const void* src, size_t bytes)
{
    if (!c) return fail(VRT_ERR_INVALID, "ctx is NULL");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return VRT_OK;
}

int vrt_memcpy_d2h(vrt_ctx* c, void* dst, const void* src, size_t bytes)
{
    if (!c) return fail(VRT_ERR_INVALID, "ctx is NULL");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return VRT_OK;
}

int vrt_memset(vrt_ctx* c, void* dst, int value, size_t bytes)
{
    if (!c) return fail(VRT_ERR_INVALID, "ctx is NULL");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemsetAsync(dst, value, bytes, c->stream));
    return VRT_OK;
}

int vrt_vox_flatten_host(const void* buf, size_t n, uint32_t dims[3], uint8_t** voxels,
                         vrt_material palette[256], uint32_t* num_instances, uint64_t* dropped)
{
    if (!buf || !dims || !voxels || !palette) return fail(VRT_ERR_INVALID, "vrt_vox_flatten_host: NULL argument");
    FlatScene fs; std::string err;
    int rc = vox_flatten((const uint8_t*)buf, n, fs, err);
    if (rc != VRT_OK) return fail(rc, err);
    dims[0] = fs.dims[0]; dims[1] = fs.dims[1]; dims[2] = fs.dims[2];
    uint8_t* v = (uint8_t*)malloc(fs.voxels.size() ? fs.voxels.size() : 1);
    if (!v) return fail(VRT_ERR_INVALID, "out of host memory");
    memcpy(v, fs.voxels.data(), fs.voxels.size());
    *voxels = v;
    memcpy(palette, fs.palette, sizeof(fs.palette));
    if (num_instances) *num_instances = fs.num_instances;
    if (dropped) *dropped = fs.dropped;
    return VRT_OK;
}

void vrt_host_free(void* p) { free(p); }

int vrt_image_load(const char* path, int* is_hdr, uint32_t* w, uint32_t* h, void** pixels)
{
    if (!path || !w || !h || !pixels) return fail(VRT_ERR_INVALID, "vrt_image_load: NULL argument");
    LoadedImage img; std::string err;
    int rc = image_load(path, img, err);
    if (rc != VRT_OK) return fail(rc, err);
    size_t bytes = img.is_hdr ? img.f32.size() * sizeof(float) : img.u8.size();
    void* p = malloc(bytes ? bytes : 1);
    if (!p) return fail(VRT_ERR_INVALID, "out of host memory");
    memcpy(p, img.is_hdr ? (const void*)img.f32.data() : (const void*)img.u8.data(), bytes);
    *pixels = p; *w = img.w; *h = img.h;
    if (is_hdr) *is_hdr = img.is_hdr ? 1 : 0;
    return VRT_OK;
}

int vrt_image_write_png(const char* path, const uint8_t* rgba8, uint32_t w, uint32_t h)
{
    if (!path || !rgba8 || !w || !h) return fail(VRT_ERR_INVALID, "vrt_image_write_png: bad argument");
    std::string err; int rc = image_write_png(path, rgba8, w, h, err);
    return rc == VRT_OK ? rc : fail(rc, err);
}

int vrt_image_write_ppm(const char* path, const uint8_t* rgba8, uint32_t w, uint32_t h)
{
    if (!path || !rgba8 || !w || !h) return fail(VRT_ERR_INVALID, "vrt_image_write_ppm: bad argument");
    std::string err; int rc = image_write_ppm(path, rgba8, w, h, err);
    return rc == VRT_OK ? rc : fail(rc, err);
}

int vrt_image_write_pfm(const char* path, const float* pixels, uint32_t w, uint32_t h, uint32_t stride_floats)
{
    if (!path || !pixels || !w || !h || stride_floats < 3) return fail(VRT_ERR_INVALID, "vrt_image_write_pfm: bad argument");
    std::string err; int rc = image_write_pfm(path, pixels, w, h, stride_floats, err);
    return rc == VRT_OK ? rc : fail(rc, err);
}

// ---- settings ------------------------------------------------------------------------------------

void vrt_settings_default(vrt_settings* s)
{
    if (!s) return;
    memset(s, 0, sizeof *s);
    s->ao_samples = 4;                       // voxel_render_settings.hpp:33
    s->ambient_intensity = 1.0f;             // :34
    const float inv = 0.57735026918962576f;  // glm::normalize(vec3(1)), :39
    s->light_dir[0] = s->light_dir[1] = s->light_dir[2] = inv;
    s->light_intensity = 1.0f;               // :41
    s->light_color[0] = s->light_color[1] = s->light_color[2] = s->light_color[3] = 1.0f;  // :40
    s->max_steps = 512;                      // voxel_volume.frag:68
    s->ao_steps = 64;                        // voxel_volume.frag:219
    s->max_bounces = 5;                      // voxel_volume.frag:69
    s->shadows = 1;
    s->traversal = VRT_TRAVERSAL_AUTO;
    s->flags = 0;
}

void vrt_denoiser_settings_default(vrt_denoiser_settings* s)
{
    if (!s) return;
    s->iterations = 2; s->phi_color0 = 20.4f; s->phi_normal0 = 1e-2f; s->phi_pos0 = 1e-1f; s->step_width = 2.0f;   // :21-29
    s->mode = VRT_DENOISE_CANONICAL;
}

} // extern "C"

// ---- shard helpers ---------------------------------------------------------------------------------

int vrt::make_shard(const vrt_shard* sh, int H, ShardMap& m, int* max_local_strips)
{
    if (!sh || sh->nranks <= 1) {
        m.rank = 0; m.nranks = 1; m.strip_rows = ceil_div(H, 16) * 16; m.n_local_strips = 1;
        m.tiles_per_strip = m.strip_rows / 16;
        if (max_local_strips) *max_local_strips = 1;
        return VRT_OK;
    }
    if (sh->rank < 0 || sh->rank >= sh->nranks || sh->strip_rows <= 0 || sh->strip_rows % 16 != 0)
        return fail(VRT_ERR_INVALID, "vrt_shard: need 0 <= rank < nranks and strip_rows a positive multiple of 16");
    int nstrips = ceil_div(H, sh->strip_rows);
    m.rank = sh->rank; m.nranks = sh->nranks; m.strip_rows = sh->strip_rows;
    m.n_local_strips = nstrips > sh->rank ? ceil_div(nstrips - sh->rank, sh->nranks) : 0;
    m.tiles_per_strip = sh->strip_rows / 16;
    if (max_local_strips) *max_local_strips = ceil_div(nstrips, sh->nranks);
    return VRT_OK;
}

// Image planes must be device memory: a host pointer handed to a kernel is a GPU fault, not an error code.  The pointer
// set of a render loop repeats from call to call, so the (comparatively slow) attribute query runs only when it changes.
int vrt::check_device_ptrs(vrt_ctx* c, int slot, const void* const* ptrs, int n, const char* what)
{
    uint64_t h = 0xcbf29ce484222325ull ^ (uint64_t)n;
    for (int i = 0; i < n; i++) { h ^= (uint64_t)(uintptr_t)ptrs[i]; h *= 0x100000001b3ull; }
    if (h == c->checked_ptrs[slot]) return VRT_OK;
    for (int i = 0; i < n; i++) {
        if (!ptrs[i]) continue;
        hipPointerAttribute_t a;
        hipError_t e = hipPointerGetAttributes(&a, ptrs[i]);
        if (e != hipSuccess) { (void)hipGetLastError(); return fail(VRT_ERR_INVALID, std::string(what) + ": image pointer is not device memory (host pointer?)"); }
        if (a.type != hipMemoryTypeDevice && a.type != hipMemoryTypeManaged)
            return fail(VRT_ERR_INVALID, std::string(what) + ": image pointer is not device memory");
    }
    c->checked_ptrs[slot] = h;
    return VRT_OK;
}

extern "C" {

int vrt_shard_rows(int32_t H, const vrt_shard* sh)
{
    ShardMap m; int mx;
    if (make_shard(sh, H, m, &mx) != VRT_OK) return -1;
    if (m.nranks == 1) return H;
    return mx * m.strip_rows;     // packed row count, identical on every rank (short ranks zero-pad)
}

// ---- geometry stage --------------------------------------------------------------------------------

// The next table of the ring, ready to be filled on the host (its previous launch, kTabRing launches ago, has finished).
static int next_table(vrt_ctx* c, int* idx)
{
    const int i = c->tab_next;
    c->tab_next = (c->tab_next + 1) % vrt_ctx::kTabRing;
    if (!c->upload_stream) HIPCHK(hipStreamCreateWithFlags(&c->upload_stream, hipStreamNonBlocking));
    if (!c->tab_dev[i]) {
        HIPCHK(c->tab_dev[i].alloc(sizeof(FrameSlot) * VRT_MAX_TABLE));
        HIPCHK(hipHostMalloc((void**)&c->tab_host[i], sizeof(FrameSlot) * VRT_MAX_TABLE, hipHostMallocDefault));
        HIPCHK(hipEventCreateWithFlags(&c->tab_uploaded[i], hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&c->tab_consumed[i], hipEventDisableTiming));
    }
    if (c->tab_busy[i]) { HIPCHK(hipEventSynchronize(c->tab_consumed[i])); c->tab_busy[i] = false; }
    *idx = i;
    return VRT_OK;
}

// One launch of K1 over n frames: n <= VRT_MAX_BATCH slots travel in the kernel arguments, more (<= VRT_MAX_TABLE) in a
// table in device memory.  shards: one strip assignment for all frames (per_frame == 0) or one per frame, all with the
// same nranks and strip_rows.  K2 follows in split mode, which renders one frame at a time.
// render_frames runs the steps below in this order: launch_args, count_planes (and the fields they need), launch_plan, the
// slots, launch_records, then the stream operations with launch_tags among them.
struct Launch {
    int n;
    const vrt_push* pushes;
    const vrt_settings* st;
    const vrt_frame* frames;
    const vrt_shard* shards;
    int per_frame;
    int W, H;                       // screen_size of frame 0, which launch_args holds every frame to
};

// The argument checks of a launch; selects the device and verifies that the image pointers are device memory.
static int launch_args(vrt_ctx* c, const vrt_scene* s, const Launch& l)
{
    const int W = l.W, H = l.H, n = l.n;
    const vrt_settings* st = l.st;
    if (W <= 0 || H <= 0 || W > 32768 || H > 32768) return fail(VRT_ERR_INVALID, "vrt_render_geometry: bad screen_size");
    if ((uint64_t)W * (uint64_t)H >= (1ull << 28))              // K1 addresses a plane with 32-bit byte offsets (16 B per pixel at most)
        return fail(VRT_ERR_UNSUPPORTED, "vrt_render_geometry: frames of 2^28 pixels and more are not supported (a launch indexes full-frame planes with "
                                         "32-bit byte offsets, sharded or not: render such an image as several frames with shifted camera planes; include/vrt.h)");
    for (int f = 0; f < n; f++) {
        const vrt_push& q = l.pushes[f];
        if (q.screen_size[0] != W || q.screen_size[1] != H)
            return fail(VRT_ERR_INVALID, "vrt_render_geometry_batch: all frames of a batch must have the same screen_size");
        if (q.volume_bounds[0] != (uint32_t)s->d.vol.W || q.volume_bounds[1] != (uint32_t)s->d.vol.H || q.volume_bounds[2] != (uint32_t)s->d.vol.D)
            return fail(VRT_ERR_INVALID, "vrt_render_geometry: push.volume_bounds must equal the scene dimensions (voxel_renderer.cpp:74)");
    }
    if (st->max_bounces > VRT_MAX_BOUNCES) return fail(VRT_ERR_INVALID, "vrt_render_geometry: max_bounces > VRT_MAX_BOUNCES");
    if (st->traversal > VRT_TRAVERSAL_DFJ) return fail(VRT_ERR_INVALID, "vrt_render_geometry: unknown traversal");
    if (s->bricks && st->traversal != VRT_TRAVERSAL_AUTO)
        return fail(VRT_ERR_UNSUPPORTED, "vrt_render_geometry: a brick scene (vrt_scene_from_bricks) renders with VRT_TRAVERSAL_AUTO only");
    if (st->traversal == VRT_TRAVERSAL_DENSE && (uint64_t)s->d.vol.W * (uint64_t)s->d.vol.H * (uint64_t)s->d.vol.D > 0xFFFFFFFFull)
        return fail(VRT_ERR_UNSUPPORTED, "vrt_render_geometry: VRT_TRAVERSAL_DENSE indexes voxels in 32 bits (volumes below 4 GiB)");
    HIPCHK(hipSetDevice(c->device));
    std::vector<const void*> ptrs((size_t)14 * (size_t)n);
    for (int f = 0; f < n; f++) {
        const vrt_frame* frame = &l.frames[f];
        const void* one[14] = {frame->color8, frame->depth, frame->motion, frame->mask8, frame->position, frame->normal8, frame->color_f,
                               frame->hit_id, frame->hit_voxel, frame->hit_mask, frame->steps_primary, frame->steps_total, frame->rays_total,
                               frame->color8_strips};
        memcpy(&ptrs[(size_t)14 * f], one, sizeof one);
    }
    return check_device_ptrs(c, 0, ptrs.data(), 14 * n, "vrt_render_geometry");
}

// Does the launch write count planes?  Such a launch reports the iterations of the reference's loop: it marches through the
// fields without open cells (with the development flags the planes hold the product march's own counters instead).
static bool count_planes(const Launch& l)
{
    bool counts = false;
    if (!(l.st->flags & (VRT_FLAG_DEBUG_PLANES | VRT_FLAG_MARCHED_COUNTS | 2u)))
        for (int f = 0; f < l.n && !counts; f++) counts = l.frames[f].steps_primary != nullptr || l.frames[f].steps_total != nullptr;
    return counts;
}

// floor(2^32 / d) for udiv_uniform (vrt_frame_slot.h), d >= 1.  For d = 1 that is 2^32, which a word does not hold -- as 0 the
// quotient came out as 1 for every n >= 2 (a frame one tile wide in a launch of nine frames or more: frames 8 .. were never
// traced); 2^32 - 1 gives n - 1 before the correction step and n after it.
static uint32_t uniform_rcp(uint32_t d)
{
    const uint64_t r = 0x100000000ull / (uint64_t)d;
    return r > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)r;
}

// The launch plan: every kernel variant, the grid and the tile map, from the context's options, the scene, the settings and the
// frames.  No HIP call and nothing of the context: what a launch takes from there (slots, records, tags, the colour table) the
// later steps put in.  count_fields: what fields_for_counts gave, or NULL; div_ok: screen_div_ok.
static int launch_plan(const DevOptions& opt, const vrt_scene* s, const Launch& l, bool counts, const uint8_t* count_fields, int div_ok,
                       GeomParams& p)
{
    const int W = l.W, H = l.H, n = l.n;
    const vrt_settings* st = l.st;
    const vrt_frame* frames = l.frames;
    memset(&p, 0, sizeof p);
    p.sc = s->d; p.st = *st;
    if (s->bricks) p.st.traversal = VRT_TRAVERSAL_BRICK;
    p.sc.vol.count_marched = (st->flags & VRT_FLAG_MARCHED_COUNTS) ? 1u : 0u;
    p.sc.vol.count_lookups = ((st->flags & VRT_FLAG_MARCHED_COUNTS) && (st->flags & VRT_FLAG_LOOKUP_COUNTS)) ? 1u : 0u;
    if (s->bricks && counts) p.sc.vol.brick_open = 0u;
    if (count_fields) p.sc.vol.df = count_fields;
    p.n_frames = n; p.W = W; p.H = H;
    p.rcp_w = 1.0f / (float)W; p.rcp_h = 1.0f / (float)H; p.fast_screen_div = div_ok;
    int max_strips = 1;
    int rc = make_shard(l.shards, H, p.sh, &max_strips);
    if (rc != VRT_OK) return rc;
    int local_strips = p.sh.n_local_strips;
    if (l.per_frame && l.shards) {
        for (int f = 1; f < n; f++) {
            ShardMap m;
            rc = make_shard(&l.shards[f], H, m, nullptr);
            if (rc != VRT_OK) return rc;
            if (m.nranks != p.sh.nranks || m.strip_rows != p.sh.strip_rows)
                return fail(VRT_ERR_INVALID, "vrt_render_geometry_slots: the frames of a launch must share nranks and strip_rows");
        }
        local_strips = p.sh.nranks > 1 ? max_strips : p.sh.n_local_strips;    // the grid covers the longest assignment
    }
    // LDS-staged traversals amortise the staging over a 16x16 tile (4 waves); the others run one 8x8 wave per workgroup,
    // which frees a wave slot the moment a wave finishes instead of when its whole tile does
    {
        uint32_t t = st->traversal;
        bool lds_mode = (t == VRT_TRAVERSAL_BITMASK || t == VRT_TRAVERSAL_JUMP);
        p.tile_w = p.tile_h = (lds_mode || (st->flags & 8u)) ? 16 : 8;
    }
    p.tiles_x = ceil_div(W, p.tile_w);
    p.tiles_y_local = local_strips * (p.sh.strip_rows / p.tile_h);
    p.total_tiles = p.tiles_x * p.tiles_y_local;
    p.chunk = p.tiles_x * ceil_div(p.tiles_y_local, 8);      // workgroups per XCD slot (tile rows are dealt round-robin)
    p.wgs_per_frame = (uint32_t)p.chunk * 8u;
    p.xcd_turn = (n > 1 && p.tiles_y_local > 0 && ceil_div(p.tiles_y_local, 8) * 8 * 100 > p.tiles_y_local * 103) ? 1 : 0;
    p.wgs_per_frame_rcp = p.wgs_per_frame ? uniform_rcp((uint32_t)p.wgs_per_frame) : 0u;
    // launches of 8 or more unsharded frames: one screen region per XCD and frame, rotating (block_to_tile, xcd_turn == 2)
    {
        const bool want = opt.xcd_regions != 0;                          // development switch
        if (want && n >= 8 && p.sh.nranks == 1 && p.tile_h == 8 && p.tiles_x >= 4 && p.tiles_y_local >= 8) {
            const uint32_t rw = ((uint32_t)p.tiles_x + 1u) / 2u, rh = ((uint32_t)p.tiles_y_local + 3u) / 4u;
            p.xcd_turn = 2;
            p.wgs_per_frame = rw * rh;
            p.wgs_per_frame_rcp = uniform_rcp((uint32_t)p.wgs_per_frame);
            p.tiles_y_rcp = uniform_rcp((uint32_t)rw);
        }
    }
    p.tps = (uint32_t)(p.sh.strip_rows / p.tile_h);
    p.tiles_x_rcp = uniform_rcp((uint32_t)p.tiles_x);
    if (p.xcd_turn != 2) p.tiles_y_rcp = p.tiles_y_local ? uniform_rcp((uint32_t)p.tiles_y_local) : 0u;
    p.tps_rcp = uniform_rcp((uint32_t)p.tps);
    // 1: nothing but primary rays; 2: megakernel (default); 0: split K1 -> records -> K2 (VRT_FLAG_SPLIT_KERNELS)
    p.fused_shade = (st->ao_samples == 0 && st->shadows == 0 && (st->max_bounces == 0 || !s->metallic_voxels)) ? 1 : ((st->flags & VRT_FLAG_SPLIT_KERNELS) ? 0 : 2);
    p.no_bounce = ((st->max_bounces == 0 || !s->metallic_voxels) && opt.no_bounce_kernel) ? 1 : 0;
    p.sc.vol.ao_batch = (opt.ao_batch && p.sc.vol.df_own) ? 1u : 0u;
    // (16 bits of a chain word count the AO rays that hit; brick scenes keep the stack of hits: the packed chain measured 6 % slower there --
    // 3.46 against 3.25 ms on config 5 -- and 1 % faster on the Mandelbulb; context option packed_bounces = 2 forces it everywhere)
    p.packed_chain = (opt.packed_bounces && st->ao_samples <= 0xFFFFu && (!s->bricks || opt.packed_bounces >= 2)) ? 1 : 0;
    // default traversal and budgets the recovery of positions from sideDist is exact for: the hand-written look-up loop
    // (vrt_march_fast.h trace_df_fast) for every ray of the frame
    {
        const bool want = opt.fast_loop != 0;                             // development switch
        const bool df = st->traversal == VRT_TRAVERSAL_AUTO || st->traversal == VRT_TRAVERSAL_DF;
        const bool sec = p.fused_shade != 1;
        bool ok = want && df && s->d.vol.df_fast && st->max_steps >= 1 && st->max_steps <= 1024 && p.tile_h == 8 &&
                  !(st->flags & (VRT_FLAG_DEBUG_PLANES | 2u)) && (!sec || st->ao_samples == 0 || (st->ao_steps >= 1 && st->ao_steps <= 1024));
        for (int f = 0; f < n && ok; f++) ok = frames[f].hit_voxel == nullptr;      // the fast loop keeps no mapPos: no hit_voxel plane
        p.fast_loop = ok ? ((counts || (st->flags & VRT_FLAG_MARCHED_COUNTS)) ? 2 : 1) : 0;      // (2: the loops' counting twins -- every launch that fills iteration-count planes)
        if (s->bricks && (counts || (st->flags & (VRT_FLAG_MARCHED_COUNTS | VRT_FLAG_DEBUG_PLANES | 2u)))) p.fast_loop = 2;      // (bricks: the march with its counters)
        // ... and the primary rays' long runs by threshold (df_prim_loop): launches that report no iteration counts (the loop keeps
        // none), axis step counts the position recovery is exact for, a budget worth not counting
        const int dmax = s->d.vol.W > s->d.vol.H ? (s->d.vol.W > s->d.vol.D ? s->d.vol.W : s->d.vol.D) : (s->d.vol.H > s->d.vol.D ? s->d.vol.H : s->d.vol.D);
        p.sc.vol.df_thresh = (ok && opt.thresh_runs && !counts && dmax <= 1022 && st->max_steps >= 32) ? 1u : 0u;
        // (brick scenes: the generic loop's form of the same, brick_march_thresh; its positions come from per-run differences)
        if (s->bricks) p.sc.vol.df_thresh = (opt.thresh_runs && !counts && !(st->flags & (VRT_FLAG_DEBUG_PLANES | 2u)) && st->max_steps >= 32) ? 1u : 0u;
    }
    // the sky texel of waves that cannot hit anything by vrt_sky.h: launches whose frames hold the reference's targets only
    // (a diagnostic plane wants values the short path does not make), pixel offsets that fit 32 bits, a sky the bound admits
    {
        bool ok = opt.sky_fast != 0 && s->d.skyk.w != 0u && !(st->flags & (VRT_FLAG_DEBUG_PLANES | 2u));
        for (int f = 0; f < n && ok; f++)
            ok = !frames[f].color_f && !frames[f].hit_voxel && !frames[f].hit_mask && !frames[f].steps_primary && !frames[f].steps_total && !frames[f].rays_total;
        p.sky_fast = ok ? 1 : 0;
    }
    p.occ2_bytes = s->occ2_bytes; p.occ3_bytes = s->occ3_bytes;
    p.occ_in_lds = ((size_t)s->occ2_bytes + s->occ3_bytes <= 65536) ? 1 : 0;
    {
        TileMap& m = p.map;
        bool six = p.sky_fast != 0;                                    // (sky_fast: no diagnostic plane, no color_f)
        for (int f = 0; f < n && six; f++)
            six = frames[f].color8 && frames[f].depth && frames[f].motion && frames[f].mask8 && frames[f].position && frames[f].normal8 &&
                  !frames[f].hit_id && !frames[f].color8_strips;
        m.flags = (st->flags & 0xFFFFu) | (p.sky_fast ? VRT_MAPFLAG_SKY_FAST : 0u) | (six ? VRT_MAPFLAG_SIX : 0u) |
                  ((p.sky_fast && opt.sky_span) ? VRT_MAPFLAG_SKY_SPAN : 0u); m.n_frames = p.n_frames; m.xcd_turn = p.xcd_turn;
        m.wgs_per_frame = p.wgs_per_frame; m.wgs_per_frame_rcp = p.wgs_per_frame_rcp;
        m.tiles_x = p.tiles_x; m.tiles_x_rcp = p.tiles_x_rcp; m.tiles_y_local = p.tiles_y_local; m.tiles_y_rcp = p.tiles_y_rcp;
        m.tps = p.tps; m.tps_rcp = p.tps_rcp; m.tile = p.tile_h; m.nranks = p.sh.nranks; m.strip_rows = p.sh.strip_rows;
        m.W = p.W; m.H = p.H;
    }
    return VRT_OK;
}

// Split launches: the context's hit records, grown to the frame, and the counter cleared.
static int launch_records(vrt_ctx* c, size_t px, GeomParams& p)
{
    if (c->records_px < px) {
        HIPCHK(hipStreamSynchronize(c->stream));
        c->records.reset(); c->hit_list.reset(); c->records_px = 0;
        HIPCHK(c->records.alloc(px * sizeof(uint4)));
        HIPCHK(c->hit_list.alloc((px + 1) * sizeof(uint32_t)));
        c->records_px = px;
    }
    p.records = c->records.get();
    p.hit_list = c->hit_list.get();
    p.hit_count = c->hit_list.get() + c->records_px;
    HIPCHK(hipMemsetAsync(p.hit_count, 0, sizeof(uint32_t), c->stream));
    return VRT_OK;
}

// Tile tags: dense scenes, frames with a box rectangle, launches that do not report the reference's iteration counts.  Takes the
// next of the context's two tag buffers (*tag_buf), grows it, and fills it: by k_tile_tags, or with the one word per frame that
// says "trace every block".  tab: the launch's slot table, or -1.
static int launch_tags(vrt_ctx* c, const vrt_scene* s, const Launch& l, const FrameSlot* slots, int tab, bool counts, const VerdictPlanes& vp,
                       GeomParams& p, int* tag_buf)
{
    const int n = l.n;
    bool want = c->opt.tile_tags != 0 && s->cells_ok && !counts && l.W <= 8128 && l.H <= 8128;
    bool any = false;
    for (int f = 0; f < n && want && !any; f++) any = !(slots[f].box[0] == 0 && slots[f].box[1] == 255 && slots[f].box[2] == 0 && slots[f].box[3] == 255);
    const bool tags = want && any;
    // (in the launch's local rows of 8x8 blocks: vrt_device.hip k_tile_tags)
    p.tags_x = tags ? (uint32_t)(p.tiles_x * (p.tile_w / 8)) : 0u; p.tags_y = tags ? (uint32_t)(p.tiles_y_local * (p.tile_h / 8)) : 0u;
    p.tags_per_frame = p.tags_x * p.tags_y + 1u;
    // (without tags: one word per frame that says "trace every block")
    const size_t words = (size_t)p.tags_per_frame * (size_t)n;
    const int b = c->tag_flip; c->tag_flip ^= 1;
    *tag_buf = b;
    if (c->tile_tags_words[b] < words) {
        HIPCHK(hipStreamSynchronize(c->stream));
        if (c->tag_stream) HIPCHK(hipStreamSynchronize(c->tag_stream));
        c->tile_tags[b].reset(); c->tile_tags_words[b] = 0;
        // (three spare words: K1 fetches the four words at a span's first block in one load -- vrt_span.h -- which in the last
        // frame's last row, or its one word without tags, reaches that far past the end; what they hold is never looked at)
        HIPCHK(c->tile_tags[b].alloc((words + 3) * sizeof(uint32_t)));
        HIPCHK(hipMemsetAsync(c->tile_tags[b].get(), 0, (words + 3) * sizeof(uint32_t), c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        c->tile_tags_words[b] = words;
        c->tag_read_valid[b] = false;
    }
    if (++c->tile_gen == 0u) {                                    // (wrapped: stale tags could match again)
        HIPCHK(hipStreamSynchronize(c->stream));
        if (c->tag_stream) HIPCHK(hipStreamSynchronize(c->tag_stream));
        for (int q = 0; q < 2; q++)
            // (the three spare words behind them are not cleared: K1 never looks at what they hold)
            if (c->tile_tags[q]) HIPCHK(hipMemsetAsync(c->tile_tags[q].get(), 0, c->tile_tags_words[q] * sizeof(uint32_t), c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        c->tile_gen = 1u;
    }
    p.tile_tags = c->tile_tags[b].get(); p.tile_gen = c->tile_gen;
    // Block verdicts for the primary-only kernels of table launches (k_block_verdicts, vrt_span.h): buffer b beside tag buffer b,
    // made behind the tags on whichever stream they are made on -- with or without tags, with or without the span path.  Launches
    // with their slots in the kernel arguments go without: their kernels work the verdicts out per wave, as before.
    if (p.fused_shade == 1 && p.table) {
        const size_t bytes = (size_t)vrt::verdict_pitch((uint32_t)(p.tiles_x * (p.tile_w / 8))) * (size_t)(p.tiles_y_local * (p.tile_h / 8)) * (size_t)n;
        if (c->verdict_bytes[b] < bytes) {
            HIPCHK(hipStreamSynchronize(c->stream));
            if (c->tag_stream) HIPCHK(hipStreamSynchronize(c->tag_stream));
            c->verdicts[b].reset(); c->verdict_bytes[b] = 0;
            // (VRT_VERDICT_HEAD bytes in front of the verdicts: the addresses of the launch's miss-colour planes, k_block_verdicts)
            HIPCHK(c->verdicts[b].alloc(VRT_VERDICT_HEAD + bytes));
            c->verdict_bytes[b] = bytes;
        }
        p.verdicts = c->verdicts[b].get() + VRT_VERDICT_HEAD;
    }
    if (!tags) {
        // every frame's one word = tile_gen
        std::vector<uint32_t> ones((size_t)n, c->tile_gen);
        HIPCHK(hipMemcpyAsync(c->tile_tags[b].get(), ones.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(launch_block_verdicts(p, vp, c->stream));
        return VRT_OK;
    }
    p.cells = s->cells.get(); p.n_cells = s->n_cells; p.cell_size = s->bricks ? 8u : 4u;
    // The tags depend on the cameras alone, not on anything the context's stream is still computing: while that stream is
    // busy (the caller runs ahead of the device: a frame loop, a batch loop) they are made on a stream of their own, under
    // the previous launch's tail, and the launch waits for an event instead of a kernel; on an idle device the second
    // stream would only add the event's latency.  (context option tags_async = 0: always on the context's stream; 2: always on
    // the second stream, busy or not -- the tests' handle on this path, which a query of the stream makes a matter of timing)
    const bool async = c->opt.tags_async >= 2 || (c->opt.tags_async != 0 && hipStreamQuery(c->stream) == hipErrorNotReady);
    if (!async) {
        HIPCHK(launch_tile_tags(p, c->stream));
        HIPCHK(launch_block_verdicts(p, vp, c->stream));
        return VRT_OK;
    }
    if (!c->tag_stream) {
        HIPCHK(hipStreamCreateWithFlags(&c->tag_stream, hipStreamNonBlocking));
        for (int q = 0; q < 2; q++) {
            HIPCHK(hipEventCreateWithFlags(&c->tag_done[q], hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&c->tag_read[q], hipEventDisableTiming));
        }
        // The launches before this one recorded no tag_read (there was no second stream to wait for it), and one of them may
        // still be reading the buffer this launch fills: the new stream starts behind everything the context's stream holds.
        HIPCHK(hipEventRecord(c->tag_read[b], c->stream));
        HIPCHK(hipStreamWaitEvent(c->tag_stream, c->tag_read[b], 0));
    }
    if (c->tag_read_valid[b]) HIPCHK(hipStreamWaitEvent(c->tag_stream, c->tag_read[b], 0));     // the launch that last read this buffer
    if (tab >= 0) HIPCHK(hipStreamWaitEvent(c->tag_stream, c->tab_uploaded[tab], 0));            // the slots the tag kernel reads
    HIPCHK(launch_tile_tags(p, c->tag_stream));
    HIPCHK(launch_block_verdicts(p, vp, c->tag_stream));
    HIPCHK(hipEventRecord(c->tag_done[b], c->tag_stream));
    HIPCHK(hipStreamWaitEvent(c->stream, c->tag_done[b], 0));
    return VRT_OK;
}

// Miss-colour planes (vrt_miss_plane.h: the rule is sky_plane_select's, this is its plumbing): the frames' keys, the rule, and
// k_miss_plane on the context's stream for every slot the rule wants filled.  vp: what k_block_verdicts hands on to K1.
static int launch_sky_planes(vrt_ctx* c, const vrt_scene* s, const Launch& l, const FrameSlot* slots, const GeomParams& p, VerdictPlanes& vp)
{
    memset(&vp, 0, sizeof vp);
    memset(c->sky_plane_last, 0, sizeof c->sky_plane_last);
    const bool eligible = p.table != nullptr && p.fused_shade == 1 && p.sky_fast != 0;
    if (!eligible || c->opt.sky_plane == 0) return VRT_OK;       // (sky_plane_select says the same; this spares the keys)
    static_assert(sizeof(RayGenConsts) == 40 && offsetof(RayGenConsts, cd) == 0, "sky_plane_key takes RayGenConsts as ten floats");
    std::vector<SkyPlaneKey> keys((size_t)l.n);
    for (int f = 0; f < l.n; f++)
        keys[(size_t)f] = sky_plane_key(reinterpret_cast<const float*>(&slots[f].rg), slots[f].pc.cam_right, l.W, l.H, p.fast_screen_div, s->shade_gen);
    SkyPlaneChoice ch;
    sky_plane_select(c->sky_planes, true, true, l.n, keys.data(), VRT_SKY_PLANE_MIN_GROUP, ch);
    const size_t px = (size_t)l.W * (size_t)l.H;
    for (int q = 0; q < VRT_SKY_PLANES; q++) {
        const int f = ch.build_from[q];
        if (f < 0) continue;
        c->sky_planes.valid[q] = false;                          // (until the kernel is in the stream: a failure below leaves no plane behind)
        if (c->sky_plane_px[q] < px) {
            HIPCHK(hipStreamSynchronize(c->stream));            // (a launch still in the stream may read the slot's old memory)
            c->sky_plane_buf[q].reset(); c->sky_plane_px[q] = 0;
            HIPCHK(c->sky_plane_buf[q].alloc(px * sizeof(uint32_t)));
            c->sky_plane_px[q] = px;
        }
        MissPlaneParams mp;
        mp.sc = p.sc; mp.rg = slots[f].rg;
        for (int a = 0; a < 3; a++) mp.cam_right[a] = slots[f].pc.cam_right[a];
        mp.rcp_w = p.rcp_w; mp.rcp_h = p.rcp_h; mp.fast_screen_div = p.fast_screen_div; mp.W = l.W; mp.H = l.H;
        mp.plane = c->sky_plane_buf[q].get();
        HIPCHK(launch_miss_plane(mp, c->stream));
        c->sky_planes.valid[q] = true;
        c->sky_planes_built++;
    }
    for (int q = 0; q < VRT_SKY_PLANES; q++) vp.plane[q] = c->sky_planes.valid[q] ? c->sky_plane_buf[q].get() : nullptr;
    for (int f = 0; f < l.n; f++) vp.which[f] = c->sky_plane_last[f] = ch.plane_of[f];
    return VRT_OK;
}

static int render_frames(vrt_ctx* c, const vrt_scene* s, int n, const vrt_push* pushes, const vrt_settings* st,
                         const vrt_frame* frames, const vrt_shard* shards, int per_frame)
{
    const Launch l = {n, pushes, st, frames, shards, per_frame, pushes[0].screen_size[0], pushes[0].screen_size[1]};
    int rc = launch_args(c, s, l);
    if (rc != VRT_OK) return rc;
    const bool counts = count_planes(l);
    const uint8_t* count_fields = nullptr;
    if (counts && !s->bricks && s->open_cells) {
        rc = fields_for_counts(c, s, &count_fields);
        if (rc != VRT_OK) return rc;
    }
    GeomParams p;
    rc = launch_plan(c->opt, s, l, counts, count_fields, screen_div_ok(c, l.W, l.H), p);
    if (rc != VRT_OK) return rc;
    FrameSlot* slots = p.slot;
    int tab = -1;
    if (n > VRT_MAX_BATCH) {
        rc = next_table(c, &tab);
        if (rc != VRT_OK) return rc;
        slots = c->tab_host[tab];
        p.table = c->tab_dev[tab].get();
    }
    const bool box_off = c->opt.box_rect == 0;                         // development switch: every wave tests the box
    for (int f = 0; f < n; f++) {
        slots[f].pc = pushes[f]; slots[f].fr = frames[f]; slots[f].rg = raygen_consts(pushes[f]);
        slots[f].shard_rank = (per_frame && shards) ? shards[f].rank : p.sh.rank;
        box_rect(pushes[f], slots[f].box);
        if (box_off) { slots[f].box[0] = slots[f].box[2] = 0; slots[f].box[1] = slots[f].box[3] = 255; }
    }
    if (!p.fused_shade) {
        rc = launch_records(c, (size_t)l.W * (size_t)l.H, p);
        if (rc != VRT_OK) return rc;
    }
    if (p.total_tiles == 0) return VRT_OK;
    // the launch sequence
    if (tab >= 0) {
        HIPCHK(hipMemcpyAsync(c->tab_dev[tab].get(), c->tab_host[tab], sizeof(FrameSlot) * (size_t)n, hipMemcpyHostToDevice, c->upload_stream));
        HIPCHK(hipEventRecord(c->tab_uploaded[tab], c->upload_stream));
        HIPCHK(hipStreamWaitEvent(c->stream, c->tab_uploaded[tab], 0));
    }
    if (c->timing) HIPCHK(hipEventRecord(c->ev_geo0, c->stream));
    // primary rays only, the reference's targets only: the hits' colours from the table (made anew when the settings or the
    // scene's sky have changed since it was made)
    if (p.fused_shade == 1 && c->opt.hit_table && p.sky_fast) {
        if (!c->hit_colors) { HIPCHK(c->hit_colors.alloc(256 * 64 * sizeof(uint32_t))); c->hit_scene_gen = 0; }
        if (c->hit_scene_gen != s->shade_gen || memcmp(&c->hit_settings, st, sizeof *st) != 0) {
            HIPCHK(launch_hit_colors(p, c->hit_colors.get(), c->stream));
            c->hit_scene_gen = s->shade_gen; c->hit_settings = *st;
        }
        p.hit_colors = c->hit_colors.get();
    }
    VerdictPlanes vp;
    rc = launch_sky_planes(c, s, l, slots, p, vp);
    if (rc != VRT_OK) return rc;
    int tag_buf = -1;
    rc = launch_tags(c, s, l, slots, tab, counts, vp, p, &tag_buf);
    if (rc != VRT_OK) return rc;
    HIPCHK(launch_primary(p, c->stream));
    if (tag_buf >= 0 && c->tag_stream) { HIPCHK(hipEventRecord(c->tag_read[tag_buf], c->stream)); c->tag_read_valid[tag_buf] = true; }
    if (tab >= 0) { HIPCHK(hipEventRecord(c->tab_consumed[tab], c->stream)); c->tab_busy[tab] = true; }
    if (c->timing) HIPCHK(hipEventRecord(c->ev_prim1, c->stream));
    if (!p.fused_shade) HIPCHK(launch_shade(p, c->stream));
    if (c->timing) { HIPCHK(hipEventRecord(c->ev_geo1, c->stream)); c->have_geo = true; }
    return VRT_OK;
}

static int render_many(vrt_ctx* c, const vrt_scene* s, int32_t n, const vrt_push* pushes, const vrt_settings* st,
                       const vrt_frame* frames, const vrt_shard* shards, int per_frame)
{
    // the split form keeps one frame's hit records: one frame per launch there
    const bool split = (st->flags & VRT_FLAG_SPLIT_KERNELS) && !(st->ao_samples == 0 && st->shadows == 0 && st->max_bounces == 0);
    const int per_launch = split ? 1 : VRT_MAX_TABLE;
    for (int f0 = 0; f0 < n; f0 += per_launch) {
        int m = n - f0 < per_launch ? n - f0 : per_launch;
        int rc = render_frames(c, s, m, pushes + f0, st, frames + f0, (per_frame && shards) ? shards + f0 : shards, per_frame);
        if (rc != VRT_OK) return rc;
    }
    return VRT_OK;
}

int vrt_render_geometry(vrt_ctx* c, const vrt_scene* s, const vrt_push* push, const vrt_settings* st,
                        const vrt_frame* frame, const vrt_shard* shard)
{
    if (!c || !s || !push || !st || !frame) return fail(VRT_ERR_INVALID, "vrt_render_geometry: NULL argument");
    return render_frames(c, s, 1, push, st, frame, shard, 0);
}

int vrt_render_geometry_batch(vrt_ctx* c, const vrt_scene* s, int32_t n, const vrt_push* pushes, const vrt_settings* st,
                              const vrt_frame* frames, const vrt_shard* shard)
{
    if (!c || !s || !pushes || !st || !frames) return fail(VRT_ERR_INVALID, "vrt_render_geometry_batch: NULL argument");
    if (n < 0) return fail(VRT_ERR_INVALID, "vrt_render_geometry_batch: n < 0");
    return render_many(c, s, n, pushes, st, frames, shard, 0);
}

int vrt_render_geometry_slots(vrt_ctx* c, const vrt_scene* s, int32_t n, const vrt_push* pushes, const vrt_settings* st,
                              const vrt_frame* frames, const vrt_shard* shards)
{
    if (!c || !s || !pushes || !st || !frames || !shards) return fail(VRT_ERR_INVALID, "vrt_render_geometry_slots: NULL argument");
    if (n < 0) return fail(VRT_ERR_INVALID, "vrt_render_geometry_slots: n < 0");
    return render_many(c, s, n, pushes, st, frames, shards, 1);
}

// The G-buffer of caller-supplied rays (kernels: vrt_render_rays.hip): the split form over a ray buffer.  Here, beside the launch
// it borrows from: the GeomParams of the shading kernel comes from launch_plan and launch_records, as a split
// vrt_render_geometry launch of one frame builds it.
int vrt_render_rays(vrt_ctx* c, const vrt_scene* s, int32_t W, int32_t H, const float* origins, const float* dirs, uint32_t frame,
                    const vrt_settings* st, const vrt_frame* out)
{
    // every argument error is reported before the context or a device is looked at
    if (!c || !s || !origins || !dirs || !st || !out) return fail(VRT_ERR_INVALID, "vrt_render_rays: NULL argument");
    if (W < 1 || H < 1 || W > 32768 || H > 32768) return fail(VRT_ERR_INVALID, "vrt_render_rays: bad frame size");
    if ((int64_t)W * (int64_t)H >= ((int64_t)1 << 28))
        return fail(VRT_ERR_INVALID, "vrt_render_rays: 2^28 pixels or more per frame (the limit of vrt_render_geometry: pass the image as several rectangles of rays)");
    if (st->max_steps == 0u) return fail(VRT_ERR_INVALID, "vrt_render_rays: max_steps == 0");
    if (st->max_bounces > VRT_MAX_BOUNCES) return fail(VRT_ERR_INVALID, "vrt_render_rays: max_bounces > VRT_MAX_BOUNCES");
    if (out->steps_primary || out->steps_total || out->rays_total || out->color8_strips)
        return fail(VRT_ERR_UNSUPPORTED, "vrt_render_rays: the count planes and color8_strips are not filled for caller-supplied rays");
    if (st->flags != 0u) return fail(VRT_ERR_UNSUPPORTED, "vrt_render_rays: settings->flags must be 0");
    if (st->traversal != VRT_TRAVERSAL_AUTO) return fail(VRT_ERR_UNSUPPORTED, "vrt_render_rays: VRT_TRAVERSAL_AUTO only");
    const size_t n = (size_t)W * (size_t)H;
    const struct { const void* p; size_t bpp; } planes[10] = {
        {out->color8, 4}, {out->depth, 4}, {out->motion, 8}, {out->mask8, 1}, {out->position, 16}, {out->normal8, 4},
        {out->color_f, 12}, {out->hit_id, 1}, {out->hit_voxel, 6}, {out->hit_mask, 1}};
    bool any = false;
    for (const auto& q : planes) any = any || q.p != nullptr;
    if (!any) return fail(VRT_ERR_INVALID, "vrt_render_rays: no output plane");
    if ((((uintptr_t)origins | (uintptr_t)dirs) & 3u) != 0u) return fail(VRT_ERR_INVALID, "vrt_render_rays: origins and dirs must be 4-byte aligned");
    for (const auto& q : planes) {
        if (!q.p) continue;
        const uintptr_t a = (uintptr_t)q.p, na = n * q.bpp;
        for (const float* r : {origins, dirs})
            if (a < (uintptr_t)r + n * 12u && (uintptr_t)r < a + na) return fail(VRT_ERR_INVALID, "vrt_render_rays: a ray plane overlaps an output plane");
    }
    HIPCHK(hipSetDevice(c->device));
    {
        const void* ptrs[12] = {origins, dirs};
        for (int q = 0; q < 10; q++) ptrs[2 + q] = planes[q].p;
        int rc = check_device_ptrs(c, 4, ptrs, 12, "vrt_render_rays");      // (a slot of its own: alternating with vrt_render_geometry keeps both digests)
        if (rc != VRT_OK) return rc;
    }
    // the synthetic push block: the shading path reads `frame` (the sample offset) and nothing else of it
    vrt_push push;
    memset(&push, 0, sizeof push);
    push.volume_bounds[0] = (uint32_t)s->d.vol.W; push.volume_bounds[1] = (uint32_t)s->d.vol.H; push.volume_bounds[2] = (uint32_t)s->d.vol.D;
    push.screen_size[0] = W; push.screen_size[1] = H; push.frame = frame;
    // the plan of a split launch of that one frame.  Of the context options "thresh_runs" and "ao_batch" are honoured, the others
    // take their defaults; hit_voxel does not choose the march here (query_recover_voxel recovers the cell on the look-up loop)
    DevOptions opt;
    opt.thresh_runs = c->opt.thresh_runs; opt.ao_batch = c->opt.ao_batch;
    vrt_settings split = *st;
    split.flags = VRT_FLAG_SPLIT_KERNELS;
    vrt_frame plan_frame = *out;
    plan_frame.hit_voxel = nullptr;
    const Launch l = {1, &push, &split, &plan_frame, nullptr, 0, W, H};
    GeomParams p;
    int rc = launch_plan(opt, s, l, false, nullptr, 0, p);
    if (rc != VRT_OK) return rc;
    p.fused_shade = 0; p.st.flags = 0u;
    p.slot[0].pc = push; p.slot[0].fr = *out; p.slot[0].rg = raygen_consts(push); p.slot[0].shard_rank = 0;
    p.slot[0].box[0] = p.slot[0].box[2] = 0; p.slot[0].box[1] = p.slot[0].box[3] = 255;
    rc = launch_records(c, n, p);
    if (rc != VRT_OK) return rc;
    // The primary march is vrt_trace_rays' (vrt_api_query.hip, query_launch): what VRT_TRAVERSAL_AUTO resolves to for the scene and
    // the budget.  The shading kernel takes the hand-written loops where the plan admits them for the secondary rays too
    // (launch_plan: the AO budget), else VRT_TRAVERSAL_DF.
    RaysParams rp;
    memset(&rp, 0, sizeof rp);
    rp.sc = p.sc; rp.origins = origins; rp.dirs = dirs; rp.fr = *out; rp.n = (uint32_t)n; rp.max_steps = st->max_steps;
    rp.records = p.records; rp.hit_list = p.hit_list; rp.hit_count = p.hit_count;
    int prim, shade;
    if (s->bricks) {
        prim = shade = VRT_TRAVERSAL_BRICK;
        rp.sc.vol.df_thresh = (c->opt.thresh_runs && st->max_steps >= 32u) ? 1u : 0u;
    } else {
        const bool fast = s->d.vol.df_fast != 0u && st->max_steps <= 1024u;
        prim = fast ? VRT_TRAVERSAL_DF_FAST : VRT_TRAVERSAL_DF;
        shade = (fast && p.fast_loop == 1) ? VRT_TRAVERSAL_DF_FAST : VRT_TRAVERSAL_DF;
        const int vw = s->d.vol.W, vh = s->d.vol.H, vd = s->d.vol.D;
        const int dmax = vw > vh ? (vw > vd ? vw : vd) : (vh > vd ? vh : vd);
        rp.sc.vol.df_thresh = (fast && c->opt.thresh_runs && dmax <= 1022 && st->max_steps >= 32u) ? 1u : 0u;
    }
    if (c->timing) HIPCHK(hipEventRecord(c->ev_geo0, c->stream));
    HIPCHK(launch_rays_primary(rp, prim, c->stream));
    if (c->timing) HIPCHK(hipEventRecord(c->ev_prim1, c->stream));
    HIPCHK(launch_rays_shade(p, dirs, rp.n, shade, c->stream));
    if (c->timing) { HIPCHK(hipEventRecord(c->ev_geo1, c->stream)); c->have_geo = true; }
    return VRT_OK;
}


// ffxFsr2GetJitterPhaseCount / ffxFsr2GetJitterOffset as documented in FidelityFX-FSR2's ffx_fsr2.h (the prebuilt
// library the reference links is absent from its tree): phase count int(8 * (display/render)^2), offset
// Halton(2,3)(index % phases + 1) - 0.5 in pixel units.  Host-only arithmetic (two floats per frame).
int32_t vrt_jitter_phase_count(int32_t render_width, int32_t display_width)
{
    if (render_width <= 0 || display_width <= 0) return 0;
    const float ratio = (float)display_width / (float)render_width;
    return (int32_t)(8.0f * (ratio * ratio));
}

static float radical_inverse(int32_t index, int32_t base)
{
    float digit = 1.0f, acc = 0.0f;
    while (index > 0) {
        digit /= (float)base;
        acc += digit * (float)(index % base);
        index /= base;
    }
    return acc;
}

int vrt_jitter_offset(int32_t index, int32_t phase_count, float* jitter_x, float* jitter_y)
{
    if (!jitter_x || !jitter_y) return fail(VRT_ERR_INVALID, "vrt_jitter_offset: NULL argument");
    if (phase_count <= 0 || index < 0) return fail(VRT_ERR_INVALID, "vrt_jitter_offset: index >= 0 and phase_count > 0 required");
    const int32_t k = index % phase_count + 1;
    *jitter_x = radical_inverse(k, 2) - 0.5f;
    *jitter_y = radical_inverse(k, 3) - 0.5f;
    return VRT_OK;
}

} // extern "C"

// ---- instrumentation -------------------------------------------------------------------------------

extern "C" {

int vrt_debug_sky_texels(vrt_ctx* c, const vrt_scene* s, const float* dirs_dev, size_t n, uint32_t* out_dev)
{
    if (!c || !s || !dirs_dev || !out_dev) return fail(VRT_ERR_INVALID, "vrt_debug_sky_texels: NULL argument");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(launch_debug_sky(s->d, dirs_dev, n, out_dev, c->stream));
    return VRT_OK;
}

int vrt_debug_spec(vrt_ctx* c, uint32_t fn, const uint32_t* a_dev, const uint32_t* b_dev, const uint32_t* c_dev, size_t n, uint32_t* out_dev)
{
    if (!c || !a_dev || !out_dev) return fail(VRT_ERR_INVALID, "vrt_debug_spec: NULL argument");
    if (fn > VRT_SPEC_NORMALIZE3) return fail(VRT_ERR_INVALID, "vrt_debug_spec: unknown fn");
    const bool two = fn == VRT_SPEC_DIV || fn == VRT_SPEC_ATAN2 || fn == VRT_SPEC_WRAP_TEXEL || fn == VRT_SPEC_NORMALIZE3;
    if ((two && !b_dev) || (fn == VRT_SPEC_NORMALIZE3 && !c_dev)) return fail(VRT_ERR_INVALID, "vrt_debug_spec: NULL argument");
    if (n > ((size_t)1 << 31)) return fail(VRT_ERR_UNSUPPORTED, "vrt_debug_spec: more than 2^31 elements");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(launch_debug_spec(fn, a_dev, b_dev, c_dev, n, out_dev, c->stream));
    return VRT_OK;
}

int vrt_debug_brick_counts(vrt_ctx* c, uint64_t out[4])
{
    if (!c || !out) return fail(VRT_ERR_INVALID, "vrt_debug_brick_counts: NULL argument");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    unsigned long long v[4];
    HIPCHK(debug_brick_counts(v));
    for (int i = 0; i < 4; i++) out[i] = v[i];
    return VRT_OK;
}

int vrt_last_timings(vrt_ctx* c, float* primary_ms, float* geometry_ms, float* denoise_ms)
{
    if (!c) return fail(VRT_ERR_INVALID, "ctx is NULL");
    HIPCHK(hipSetDevice(c->device));
    if (primary_ms) *primary_ms = -1.0f;
    if (geometry_ms) *geometry_ms = -1.0f;
    if (denoise_ms) *denoise_ms = -1.0f;
    if (c->have_geo) {
        HIPCHK(hipEventSynchronize(c->ev_geo1));
        if (primary_ms) HIPCHK(hipEventElapsedTime(primary_ms, c->ev_geo0, c->ev_prim1));
        if (geometry_ms) HIPCHK(hipEventElapsedTime(geometry_ms, c->ev_geo0, c->ev_geo1));
    }
    if (c->have_den) {
        HIPCHK(hipEventSynchronize(c->ev_den1));
        if (denoise_ms) HIPCHK(hipEventElapsedTime(denoise_ms, c->ev_den0, c->ev_den1));
    }
    return VRT_OK;
}

} // extern "C"

