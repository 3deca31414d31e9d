// vrt_raygen.h -- ray generators (vrt_camera_rays): the primary ray of pixel (px, py) of a W x H frame under three camera
// models, step by step.  This file is the definition: k_camera_rays (vrt_rays.hip) evaluates camera_ray() on the device,
// tests/native/raygen_host.cpp on the host, and tests/raygen_reference.py restates it in numpy; all three agree bit for bit.
//
// Everything per pixel is fp32, evaluated in the written order without FMA contraction (-ffp-contract=off), with IEEE
// division and square root, and without a transcendental function: what needs one (the tangent of half the field of view,
// the panorama's sines and cosines) the host computes once per call in double and rounds once (raygen_consts_of,
// panorama_tables).
//
// Screen coordinates, all models (voxel_volume.frag:312-313 through screen_quad.vert):
//     sx = ((px + 0.5) / W) * 2 - 1          sy = ((py + 0.5) / H) * 2 - 1
//
// VRT_CAMERA_PERSPECTIVE -- main()'s pinhole (frag:312-322) with a field of view:
//     cd  = normalize(cam_dir)               (the reference re-normalises camDir, so its length -- the focal length -- is lost)
//     U   = cam_right * tan_half             V = ((cam_up * tan_half) * H) / W
//     J   = (camera_jitter.x / W * -2, camera_jitter.y / H * 2, 0)
//     v   = ((cd + sx * U) + sy * V) + J
//     dir = normalize(v)                     origin = cam_pos
//   tan_half = tan(horizontal FOV / 2).  With tan_half == 1.0f this is main()'s ray bit for bit: x * 1.0f == x.
//
// VRT_CAMERA_ORTHOGRAPHIC -- parallel rays:
//     U   = cam_right * half_width           V = ((cam_up * half_width) * H) / W
//     dir = cd                               origin = (cam_pos + sx * U) + sy * V
//   half_width: half the width of the view, in voxels.  The jitter is not applied.
//
// VRT_CAMERA_PANORAMA -- equirectangular, the inverse of skyColor's mapping (frag:98-105: u = atan(d.z, d.x) * 0.1591 + 0.5,
// t = asin(-d.y) * 0.3183 + 0.5):
//     u = (px + 0.5) / W    theta = (u - 0.5) / 0.1591          col[px] = (cos theta, sin theta)
//     t = (py + 0.5) / H    phi   = (t - 0.5) / 0.3183          row[py] = (cos phi, sin phi)
//     dir = (cos phi * cos theta, -sin phi, cos phi * sin theta)      origin = cam_pos
//   The tables are computed in double -- the two constants are the shader's fp32 ones, widened -- and rounded once to fp32;
//   the per-pixel function only multiplies.  The basis and the jitter are not used: the panorama looks along the volume's axes.
#pragma once

#include "vrt_spec.h"
#include "../../include/vrt.h"

namespace vrt {

// the pixel-independent part of a camera, made once per call on the host
struct RayCamConsts {
    int32_t model;
    int32_t W, H;
    float   Wf, Hf;
    f3      cd, U, V, pos;
    float   jx, jy;
};

inline bool raygen_finite(float x) { return x - x == 0.0f; }

// 0: ok; 1: unknown model; 2: bad tan_half / half_width; 3: degenerate basis
inline int raygen_consts_of(const vrt_ray_camera& cam, int32_t W, int32_t H, RayCamConsts& k)
{
    const vrt_push& pc = cam.basis;
    k.model = cam.model; k.W = W; k.H = H; k.Wf = (float)W; k.Hf = (float)H;
    k.pos = mk3(pc.cam_pos[0], pc.cam_pos[1], pc.cam_pos[2]);
    k.cd = k.U = k.V = mk3(0.0f, 0.0f, 0.0f);
    k.jx = k.jy = 0.0f;
    if (cam.model != VRT_CAMERA_PERSPECTIVE && cam.model != VRT_CAMERA_ORTHOGRAPHIC && cam.model != VRT_CAMERA_PANORAMA) return 1;
    if (!raygen_finite(k.pos.x) || !raygen_finite(k.pos.y) || !raygen_finite(k.pos.z)) return 3;
    if (cam.model == VRT_CAMERA_PANORAMA) return 0;
    const float scale = cam.model == VRT_CAMERA_PERSPECTIVE ? cam.tan_half : cam.half_width;
    if (!(scale > 0.0f) || !raygen_finite(scale)) return 2;
    k.cd = normalize3(mk3(pc.cam_dir[0], pc.cam_dir[1], pc.cam_dir[2]));
    k.U = mk3(pc.cam_right[0] * scale, pc.cam_right[1] * scale, pc.cam_right[2] * scale);
    k.V = mk3(((pc.cam_up[0] * scale) * k.Hf) / k.Wf, ((pc.cam_up[1] * scale) * k.Hf) / k.Wf, ((pc.cam_up[2] * scale) * k.Hf) / k.Wf);
    if (cam.model == VRT_CAMERA_PERSPECTIVE) {
        k.jx = (pc.camera_jitter[0] / k.Wf) * -2.0f;
        k.jy = (pc.camera_jitter[1] / k.Hf) * 2.0f;
        if (!raygen_finite(k.jx) || !raygen_finite(k.jy)) return 3;
    }
    // the three vectors span space: a non-zero, finite determinant (in double: no overflow of products of finite floats)
    const double a[3] = {k.U.x, k.U.y, k.U.z}, b[3] = {k.V.x, k.V.y, k.V.z}, c[3] = {k.cd.x, k.cd.y, k.cd.z};
    const double det = a[0] * (b[1] * c[2] - b[2] * c[1]) - b[0] * (a[1] * c[2] - a[2] * c[1]) + c[0] * (a[1] * b[2] - a[2] * b[1]);
    if (!(det != 0.0) || !(det - det == 0.0)) return 3;
    return 0;
}

// the panorama's tables: col[2 px] = cos theta, col[2 px + 1] = sin theta (W pairs); row[2 py] = cos phi, row[2 py + 1] = sin phi
inline void panorama_tables(int32_t W, int32_t H, float* col, float* row)
{
    const double ku = (double)0.1591f, kv = (double)0.3183f;
    for (int32_t px = 0; px < W; px++) {
        const double th = (((double)px + 0.5) / (double)W - 0.5) / ku;
        col[2 * px] = (float)cos(th); col[2 * px + 1] = (float)sin(th);
    }
    for (int32_t py = 0; py < H; py++) {
        const double ph = (((double)py + 0.5) / (double)H - 0.5) / kv;
        row[2 * py] = (float)cos(ph); row[2 * py + 1] = (float)sin(ph);
    }
}

// the ray of pixel (px, py); col, row: the panorama's tables (unused by the other models)
VRT_HD void camera_ray(const RayCamConsts& k, const float* col, const float* row, int px, int py, f3& origin, f3& dir)
{
    if (k.model == VRT_CAMERA_PANORAMA) {
        const float ct = col[2 * px], st = col[2 * px + 1], cp = row[2 * py], sp = row[2 * py + 1];
        dir = mk3(cp * ct, -sp, cp * st);
        origin = k.pos;
        return;
    }
    const float sx = (((float)px + 0.5f) / k.Wf) * 2.0f - 1.0f;
    const float sy = (((float)py + 0.5f) / k.Hf) * 2.0f - 1.0f;
    if (k.model == VRT_CAMERA_ORTHOGRAPHIC) {
        dir = k.cd;
        origin = mk3((k.pos.x + sx * k.U.x) + sy * k.V.x, (k.pos.y + sx * k.U.y) + sy * k.V.y, (k.pos.z + sx * k.U.z) + sy * k.V.z);
        return;
    }
    const float vx = ((k.cd.x + sx * k.U.x) + sy * k.V.x) + k.jx;
    const float vy = ((k.cd.y + sx * k.U.y) + sy * k.V.y) + k.jy;
    const float vz = ((k.cd.z + sx * k.U.z) + sy * k.V.z) + 0.0f;
    dir = normalize3(mk3(vx, vy, vz));
    origin = k.pos;
}

// ---- sub-pixel sample offsets (vrt_camera_rays_offset) ---------------------------------------------------------------------------
// The rays through the points (px + 0.5 + ox, py + 0.5 + oy) of the pixel grid, ox and oy in pixels, |o| <= 1: what gives the
// orthographic and the panorama model -- which apply no jitter -- samples that fall between each other from frame to frame, for
// vrt_upsample_camera to gather.  camera_ray is not touched; camera_ray_offset is its text with
//     sx = ((((float)px + 0.5f) + ox) / W) * 2 - 1          sy = ((((float)py + 0.5f) + oy) / H) * 2 - 1
// (the perspective model's own J still added), and the panorama's tables computed in double at px + 0.5 + ox and py + 0.5 + oy.
// With (ox, oy) == (0, 0) every ray equals camera_ray's bit for bit: x + 0.0f == x for the positive x here.

inline void panorama_tables_offset(int32_t W, int32_t H, float ox, float oy, float* col, float* row)
{
    const double ku = (double)0.1591f, kv = (double)0.3183f;
    for (int32_t px = 0; px < W; px++) {
        const double th = ((((double)px + 0.5) + (double)ox) / (double)W - 0.5) / ku;
        col[2 * px] = (float)cos(th); col[2 * px + 1] = (float)sin(th);
    }
    for (int32_t py = 0; py < H; py++) {
        const double ph = ((((double)py + 0.5) + (double)oy) / (double)H - 0.5) / kv;
        row[2 * py] = (float)cos(ph); row[2 * py + 1] = (float)sin(ph);
    }
}

// the ray of pixel (px, py) through (px + 0.5 + ox, py + 0.5 + oy); col, row: panorama_tables_offset's (unused by the other models)
VRT_HD void camera_ray_offset(const RayCamConsts& k, const float* col, const float* row, float ox, float oy, int px, int py,
                              f3& origin, f3& dir)
{
    if (k.model == VRT_CAMERA_PANORAMA) {
        const float ct = col[2 * px], st = col[2 * px + 1], cp = row[2 * py], sp = row[2 * py + 1];
        dir = mk3(cp * ct, -sp, cp * st);
        origin = k.pos;
        return;
    }
    const float sx = ((((float)px + 0.5f) + ox) / k.Wf) * 2.0f - 1.0f;
    const float sy = ((((float)py + 0.5f) + oy) / k.Hf) * 2.0f - 1.0f;
    if (k.model == VRT_CAMERA_ORTHOGRAPHIC) {
        dir = k.cd;
        origin = mk3((k.pos.x + sx * k.U.x) + sy * k.V.x, (k.pos.y + sx * k.U.y) + sy * k.V.y, (k.pos.z + sx * k.U.z) + sy * k.V.z);
        return;
    }
    const float vx = ((k.cd.x + sx * k.U.x) + sy * k.V.x) + k.jx;
    const float vy = ((k.cd.y + sx * k.U.y) + sy * k.V.y) + k.jy;
    const float vz = ((k.cd.z + sx * k.U.z) + sy * k.V.z) + 0.0f;
    dir = normalize3(mk3(vx, vy, vz));
    origin = k.pos;
}

} // namespace vrt
