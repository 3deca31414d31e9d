// reproject_host.cpp -- TEST HELPER: the per-pixel function of temporal reprojection (csrc/vrt_reproject.h) compiled for the
// host, so that the definition the kernel runs can be compared with its numpy restatement (tests/reproject_reference.py)
// without a GPU.  Built on demand by tests/test_reproject_cpu.py (g++ -ffp-contract=off).
#include "../../include/vrt.h"
#include "../../voxel-raytracing_amd/csrc/vrt_reproject.h"

using namespace vrt;

extern "C" {

// One frame over host planes, the loop vrt_reproject's kernel runs one thread per pixel of.  hist_color / hist_surface: both
// NULL to start a new sequence; resolved8 / motion may be NULL.  Returns 0, or 1 where vrt_reproject answers VRT_ERR_INVALID
// for the previous camera's basis.
int rh_reproject(int W, int H, const vrt_push* cur, const vrt_push* prev, uint32_t max_history, float tol_abs, float tol_rel,
                 const uint32_t* color8, const uint32_t* position, const uint32_t* normal8,
                 const uint32_t* hist_color, const uint32_t* hist_surface,
                 uint32_t* out_color, uint32_t* out_surface, uint32_t* resolved8, float* motion)
{
    ReprojectConsts k;
    if (!reproject_consts(W, H, prev->cam_pos, prev->cam_dir, prev->cam_right, prev->cam_up, prev->camera_jitter, cur->cam_pos,
                          tol_abs, tol_rel, max_history, k))
        return 1;
    for (int py = 0; py < H; py++)
        for (int px = 0; px < W; px++) {
            const size_t i = (size_t)py * W + px;
            rp_u4 P4; P4.x = position[4 * i]; P4.y = position[4 * i + 1]; P4.z = position[4 * i + 2]; P4.w = position[4 * i + 3];
            ReprojectPixel o;
            reproject_pixel(k, px, py, P4, normal8[i], color8[i], (const rp_u4*)hist_surface, (const rp_u2*)hist_color, o);
            out_color[2 * i] = o.color16.x; out_color[2 * i + 1] = o.color16.y;
            out_surface[4 * i] = o.surface.x; out_surface[4 * i + 1] = o.surface.y; out_surface[4 * i + 2] = o.surface.z; out_surface[4 * i + 3] = o.surface.w;
            if (resolved8) resolved8[i] = o.resolved;
            if (motion) { motion[2 * i] = o.mvx; motion[2 * i + 1] = o.mvy; }
        }
    return 0;
}

float rh_default_tol_rel(const vrt_push* cur, int W) { return reproject_default_tol_rel(cur->cam_right, W); }

size_t rh_sizeof_history() { return sizeof(vrt_history); }
size_t rh_sizeof_settings() { return sizeof(vrt_reproject_settings); }

} // extern "C"
