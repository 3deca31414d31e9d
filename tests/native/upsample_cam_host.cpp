// upsample_cam_host.cpp -- TEST HELPER: the per-pixel function of temporal upsampling for ray cameras (csrc/vrt_upsample_cam.h) and
// the ray generator with a sub-pixel offset (csrc/vrt_raygen.h: camera_ray_offset) compiled for the host, so that the definitions
// the kernels run can be compared with their numpy restatement (tests/upsample_cam_reference.py) without a GPU.  Built on demand by
// tests/upsample_cam_common.py (g++ -ffp-contract=off).
#include <vector>

#include "../../include/vrt.h"
#include "../../voxel-raytracing_amd/csrc/vrt_upsample_cam.h"

using namespace vrt;

extern "C" {

// One frame over host planes, the loop vrt_upsample_camera's kernel runs one thread per display pixel of.  hist_color /
// hist_surface: both NULL to start a new sequence; resolved8 / motion may be NULL.  Returns 0, or upsample_cam_consts' code where
// vrt_upsample_camera answers VRT_ERR_INVALID for the cameras.
int uch_upsample(int w, int h, int TW, int TH, const vrt_ray_camera* cur, const vrt_ray_camera* prev, uint32_t max_history,
                 float tol_abs, float tol_rel, const uint32_t* color8, const uint32_t* position, const uint32_t* normal8,
                 const uint32_t* hist_color, const uint32_t* hist_surface, uint32_t* out_color, uint32_t* out_surface,
                 uint32_t* resolved8, float* motion)
{
    UpsampleCamConsts k;
    const int bad = upsample_cam_consts(w, h, TW, TH, *cur, *prev, tol_abs, tol_rel, max_history, k);
    if (bad) return bad;
    for (int Y = 0; Y < TH; Y++)
        for (int X = 0; X < TW; X++) {
            int rx, ry;
            upsample_source(k.k, X, Y, rx, ry);
            const size_t j = (size_t)ry * w + rx, i = (size_t)Y * TW + X;
            rp_u4 P4; P4.x = position[4 * j]; P4.y = position[4 * j + 1]; P4.z = position[4 * j + 2]; P4.w = position[4 * j + 3];
            ReprojectPixel o;
            upsample_cam_pixel_of(k, X, Y, P4, normal8[j], color8[j], (const rp_u4*)hist_surface, (const rp_u2*)hist_color, o);
            out_color[2 * i] = o.color16.x; out_color[2 * i + 1] = o.color16.y;
            out_surface[4 * i] = o.surface.x; out_surface[4 * i + 1] = o.surface.y; out_surface[4 * i + 2] = o.surface.z; out_surface[4 * i + 3] = o.surface.w;
            if (resolved8) resolved8[i] = o.resolved;
            if (motion) { motion[2 * i] = o.mvx; motion[2 * i + 1] = o.mvy; }
        }
    return 0;
}

float uch_default_tol_rel(const vrt_ray_camera* cur, int w) { return reproject_cam_default_tol_rel(*cur, w); }

// The rays of a W x H frame through (px + 0.5 + ox, py + 0.5 + oy): origins then dirs, W * H x 3 floats each.  Returns
// raygen_consts_of's code.
int uch_rays_offset(const vrt_ray_camera* cam, int W, int H, float ox, float oy, float* origins, float* dirs)
{
    RayCamConsts k;
    const int rc = raygen_consts_of(*cam, W, H, k);
    if (rc != 0) return rc;
    std::vector<float> col(2 * (size_t)W), row(2 * (size_t)H);
    if (k.model == VRT_CAMERA_PANORAMA) panorama_tables_offset(W, H, ox, oy, col.data(), row.data());
    for (int py = 0; py < H; py++)
        for (int px = 0; px < W; px++) {
            f3 ro, rd;
            camera_ray_offset(k, col.data(), row.data(), ox, oy, px, py, ro, rd);
            const size_t i = ((size_t)py * (size_t)W + (size_t)px) * 3;
            origins[i] = ro.x; origins[i + 1] = ro.y; origins[i + 2] = ro.z;
            dirs[i] = rd.x; dirs[i + 1] = rd.y; dirs[i + 2] = rd.z;
        }
    return 0;
}

// upsample_cam_project of n world points (xyz each) through cam, as the current camera of a w x h -> TW x TH call: front[i] and,
// where it is 1, xy[2 i], xy[2 i + 1].  Returns upsample_cam_consts' code.
int uch_project(const vrt_ray_camera* cam, int w, int h, int TW, int TH, int n, const float* P, uint8_t* front, float* xy)
{
    UpsampleCamConsts k;
    const int bad = upsample_cam_consts(w, h, TW, TH, *cam, *cam, 0.5f, 0.0f, 1u, k);
    if (bad) return bad;
    for (int i = 0; i < n; i++) {
        const f3 p = mk3(P[3 * i], P[3 * i + 1], P[3 * i + 2]);
        float x = 0.0f, y = 0.0f;
        bool f;
        if (k.model == VRT_CAMERA_PANORAMA) f = upsample_cam_project<VRT_CAMERA_PANORAMA>(k.k.cur, k.k.TW, k.k.TH, p, x, y);
        else if (k.model == VRT_CAMERA_ORTHOGRAPHIC) f = upsample_cam_project<VRT_CAMERA_ORTHOGRAPHIC>(k.k.cur, k.k.TW, k.k.TH, p, x, y);
        else f = upsample_cam_project<VRT_CAMERA_PERSPECTIVE>(k.k.cur, k.k.TW, k.k.TH, p, x, y);
        front[i] = f ? 1 : 0; xy[2 * i] = x; xy[2 * i + 1] = y;
    }
    return 0;
}

size_t uch_sizeof_camera() { return sizeof(vrt_ray_camera); }

} // extern "C"
