// vrt_api_rays.hip -- ray generation of the C-ABI (vrt_camera_rays, vrt_camera_rays_offset); the kernels are vrt_rays.hip, the
// camera models csrc/vrt_raygen.h.
#include "vrt_host.h"

using namespace vrt;

namespace {

// W x H within vrt_render_geometry's limits (a launch addresses full-frame planes with 32-bit byte offsets, 16 B per pixel at most)
int frame_size(const char* who, int32_t W, int32_t H)
{
    if (W < 1 || H < 1 || W > 32768 || H > 32768) return fail(VRT_ERR_INVALID, std::string(who) + ": bad frame size");
    if ((int64_t)W * (int64_t)H >= ((int64_t)1 << 28))
        return fail(VRT_ERR_INVALID, std::string(who) + ": 2^28 pixels or more per frame (the limit of vrt_render_geometry: pass the image as several rectangles of rays)");
    return VRT_OK;
}

bool overlaps(const void* a, size_t na, const void* b, size_t nb)
{
    return (uintptr_t)a < (uintptr_t)b + nb && (uintptr_t)b < (uintptr_t)a + na;
}

// the panorama's tables in device memory: 2 (W + H) floats, owned by the context, with a pinned host image to copy from.  A
// second panorama call waits for the first one's kernel before it refills them.
int upload_panorama(vrt_ctx* c, int32_t W, int32_t H, const float* offset, const float** col, const float** row)
{
    const size_t n = 2 * ((size_t)W + (size_t)H);
    if (c->pano_busy) { HIPCHK(hipEventSynchronize(c->pano_done)); c->pano_busy = false; }
    if (c->pano_floats < n) {
        if (c->pano_host) { HIPCHK(hipHostFree(c->pano_host)); c->pano_host = nullptr; }
        c->pano_dev.reset(); c->pano_floats = 0;
        HIPCHK(c->pano_dev.alloc(n * sizeof(float)));
        HIPCHK(hipHostMalloc((void**)&c->pano_host, n * sizeof(float), hipHostMallocDefault));
        c->pano_floats = n;
    }
    if (!c->pano_done) HIPCHK(hipEventCreateWithFlags(&c->pano_done, hipEventDisableTiming));
    if (offset) panorama_tables_offset(W, H, offset[0], offset[1], c->pano_host, c->pano_host + 2 * (size_t)W);
    else panorama_tables(W, H, c->pano_host, c->pano_host + 2 * (size_t)W);
    HIPCHK(hipMemcpyAsync(c->pano_dev.get(), c->pano_host, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    *col = c->pano_dev.get(); *row = c->pano_dev.get() + 2 * (size_t)W;
    return VRT_OK;
}

// vrt_camera_rays (offset == nullptr: camera_ray, k_camera_rays) and vrt_camera_rays_offset (camera_ray_offset,
// k_camera_rays_offset): one set of argument rules, reported under the entry point's name
int camera_rays_call(const char* who, vrt_ctx* c, const vrt_ray_camera* cam, int32_t W, int32_t H, const float* offset, float* origins,
                     float* dirs)
{
    const std::string fn(who);
    // every argument error is reported before the context or a device is looked at
    if (!c || !cam || !origins || !dirs) return fail(VRT_ERR_INVALID, fn + ": NULL argument");
    int rc = frame_size(who, W, H);
    if (rc != VRT_OK) return rc;
    RayCamConsts k;
    const int bad = raygen_consts_of(*cam, W, H, k);
    if (bad == 1) return fail(VRT_ERR_INVALID, fn + ": unknown camera model");
    if (bad == 2) return fail(VRT_ERR_INVALID, fn + (cam->model == VRT_CAMERA_PERSPECTIVE ? ": tan_half must be finite and positive"
                                                                                           : ": half_width must be finite and positive"));
    if (bad) return fail(VRT_ERR_INVALID, fn + ": the camera's basis is degenerate (a non-finite position or jitter, a zero or non-finite determinant)");
    const size_t bytes = (size_t)W * (size_t)H * 12u;
    if ((((uintptr_t)origins | (uintptr_t)dirs) & 3u) != 0u) return fail(VRT_ERR_INVALID, fn + ": origins and dirs must be 4-byte aligned");
    if (overlaps(origins, bytes, dirs, bytes)) return fail(VRT_ERR_INVALID, fn + ": origins and dirs overlap");
    HIPCHK(hipSetDevice(c->device));
    const void* ptrs[2] = {origins, dirs};
    rc = check_device_ptrs(c, 3, ptrs, 2, who);
    if (rc != VRT_OK) return rc;
    const float* col = nullptr; const float* row = nullptr;
    if (k.model == VRT_CAMERA_PANORAMA) {
        rc = upload_panorama(c, W, H, offset, &col, &row);
        if (rc != VRT_OK) return rc;
    }
    if (offset) HIPCHK(launch_camera_rays_offset(k, col, row, offset[0], offset[1], origins, dirs, c->stream));
    else HIPCHK(launch_camera_rays(k, col, row, origins, dirs, c->stream));
    if (k.model == VRT_CAMERA_PANORAMA) { HIPCHK(hipEventRecord(c->pano_done, c->stream)); c->pano_busy = true; }
    return VRT_OK;
}

} // namespace

extern "C" {

int vrt_camera_rays(vrt_ctx* c, const vrt_ray_camera* cam, int32_t W, int32_t H, float* origins, float* dirs)
{
    return camera_rays_call("vrt_camera_rays", c, cam, W, H, nullptr, origins, dirs);
}

int vrt_camera_rays_offset(vrt_ctx* c, const vrt_ray_camera* cam, int32_t W, int32_t H, const float offset[2], float* origins, float* dirs)
{
    if (!offset) return fail(VRT_ERR_INVALID, "vrt_camera_rays_offset: NULL argument");
    if (!raygen_finite(offset[0]) || !raygen_finite(offset[1]) || !(fabsf(offset[0]) <= 1.0f) || !(fabsf(offset[1]) <= 1.0f))
        return fail(VRT_ERR_INVALID, "vrt_camera_rays_offset: the offset must be finite and within one pixel (|o| <= 1)");
    return camera_rays_call("vrt_camera_rays_offset", c, cam, W, H, offset, origins, dirs);
}

} // extern "C"
