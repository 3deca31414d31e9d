// reproject_cam_host.cpp -- TEST HELPER: the per-pixel function of temporal reprojection for ray cameras
// (csrc/vrt_reproject_cam.h) compiled for the host, so that the definition the kernel runs can be compared with its numpy
// restatement (tests/reproject_cam_reference.py) without a GPU.  Built on demand by tests/test_reproject_cam_cpu.py
// (g++ -ffp-contract=off).
#include "../../include/vrt.h"
#include "../../voxel-raytracing_amd/csrc/vrt_reproject_cam.h"

using namespace vrt;

extern "C" {

// One frame over host planes, the loop vrt_reproject_camera's kernel runs one thread per pixel of.  hist_color / hist_surface:
// both NULL to start a new sequence; resolved8 / motion may be NULL.  Returns 0, or reproject_cam_consts' code where
// vrt_reproject_camera answers VRT_ERR_INVALID for the cameras.
int rch_reproject(int W, int H, const vrt_ray_camera* cur, const vrt_ray_camera* prev, uint32_t max_history, float tol_abs,
                  float tol_rel, const uint32_t* color8, const uint32_t* position, const uint32_t* normal8,
                  const uint32_t* hist_color, const uint32_t* hist_surface,
                  uint32_t* out_color, uint32_t* out_surface, uint32_t* resolved8, float* motion)
{
    ReprojectCamConsts k;
    const int bad = reproject_cam_consts(W, H, *cur, *prev, tol_abs, tol_rel, max_history, k);
    if (bad) return bad;
    for (int py = 0; py < H; py++)
        for (int px = 0; px < W; px++) {
            const size_t i = (size_t)py * W + px;
            rp_u4 P4; P4.x = position[4 * i]; P4.y = position[4 * i + 1]; P4.z = position[4 * i + 2]; P4.w = position[4 * i + 3];
            ReprojectPixel o;
            reproject_cam_pixel_of(k, px, py, P4, normal8[i], color8[i], (const rp_u4*)hist_surface, (const rp_u2*)hist_color, o);
            out_color[2 * i] = o.color16.x; out_color[2 * i + 1] = o.color16.y;
            out_surface[4 * i] = o.surface.x; out_surface[4 * i + 1] = o.surface.y; out_surface[4 * i + 2] = o.surface.z; out_surface[4 * i + 3] = o.surface.w;
            if (resolved8) resolved8[i] = o.resolved;
            if (motion) { motion[2 * i] = o.mvx; motion[2 * i + 1] = o.mvy; }
        }
    return 0;
}

float rch_default_tol_rel(const vrt_ray_camera* cur, int W) { return reproject_cam_default_tol_rel(*cur, W); }

size_t rch_sizeof_camera() { return sizeof(vrt_ray_camera); }

} // extern "C"
