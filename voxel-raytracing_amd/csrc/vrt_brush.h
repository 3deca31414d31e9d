// vrt_brush.h -- which voxels a brush covers and what they become (vrt_scene_brush), and how a stamp maps a box of one scene onto
// another (vrt_scene_stamp).  Plain integer arithmetic, no floating point anywhere: coverage is a function of integers, so the
// device (vrt_brush.hip), the host (vrt_api_edit.hip) and the tests (tests/native/brush_host.cpp, brush_fuzz.cpp, held against
// Python integers) agree bit for bit by construction.
//
// UNITS.  Shape positions are in HALF VOXELS (int32): the centre of voxel (x, y, z) is P = (2x+1, 2y+1, 2z+1), so a brush can
// be centred on a voxel (odd coordinates) or on a voxel corner (even ones).
//
// SHAPES (vrt_brush::p, nine int32):
//   VRT_BRUSH_BOX        p[0..2] = lo, p[3..5] = size, in VOXELS; lo may be negative, every size in 1..2^30.
//                        Inside iff lo <= (x, y, z) < lo + size.
//   VRT_BRUSH_ELLIPSOID  p[0..2] = centre c, p[3..5] = semi-axes r, in half voxels; every r in 1..1024.  With d = P - c:
//                        inside iff dx^2 ry^2 rz^2 + dy^2 rx^2 rz^2 + dz^2 rx^2 ry^2 <= rx^2 ry^2 rz^2.
//                        A sphere has equal semi-axes; r = (1, 1, 1) centred on a voxel is that one voxel.
//   VRT_BRUSH_CAPSULE    p[0..2] = a, p[3..5] = b, p[6] = r, in half voxels; r in 1..1024, every coordinate of a and b in
//                        -4096..12288.  With e = b - a, L2 = |e|^2, q = (P - a) . e:
//                          q <= 0 or L2 == 0:  inside iff |P - a|^2 <= r^2          (a == b is a sphere: this branch, no division)
//                          q >= L2:            inside iff |P - b|^2 <= r^2
//                          otherwise:          inside iff |P - a|^2 L2 - q^2 <= r^2 L2
// brush_bounds gives the voxel box [lo, hi) that holds every covered voxel (per axis the voxels whose centre lies within the
// shape's extent); brush_inside answers false outside it without evaluating a product, so inside it -- where the products are
// evaluated -- every one fits int64:
//   ellipsoid  |d_a| <= r_a <= 2^10, so each term d_a^2 r_b^2 r_c^2 <= 2^60, their sum <= 3 * 2^60 < 2^62, the right side <= 2^60.
//   capsule    |e_a| <= 16384 = 2^14, |P_a - a_a| and |P_a - b_a| <= 16384 + 1024 = 17408 < 2^15.
//              L2 <= 3 * 2^28 < 2^30;  |P - a|^2, |P - b|^2 <= 3 * 17408^2 = 909 115 392 < 2^30;  |q| <= 3 * 17408 * 16384 < 2^30.
//              |P - a|^2 L2 < 2^60, q^2 < 2^60, their difference is >= 0 (Cauchy-Schwarz) and < 2^60;  r^2 L2 < 2^50.
//   box        lo + size in int64: |lo| <= 2^31, size <= 2^30.
//
// MODES.  brush_value says what a voxel INSIDE the shape becomes (outside it keeps `old`):
//   VRT_BRUSH_SET      id                          (0 carves)
//   VRT_BRUSH_PAINT    old != 0 ? id : old         id != 0
//   VRT_BRUSH_ADD      old == 0 ? id : old         id != 0
//   VRT_BRUSH_REPLACE  old == match ? id : old     id != match
// A voxel that changes therefore always becomes `id`.
//
// CLIPPING.  brush_clip intersects the bounds with the volume: a brush partly outside covers what is inside, one wholly outside
// covers nothing (and is no error -- unlike vrt_scene_edit_box, which refuses a box that leaves the volume).
//
// STAMPS.  An orientation is perm | flips << 3.  perm in 0..5 says which SOURCE axis feeds each DESTINATION axis:
//     perm   dst x  dst y  dst z
//      0       x      y      z          (stamp_perm_axis)
//      1       x      z      y
//      2       y      x      z
//      3       y      z      x
//      4       z      x      y
//      5       z      y      x
// and bit a of flips (0..7) reverses destination axis a.  The oriented box has the sides stamp_dst_size; destination offset
// (dx, dy, dz) inside it takes the source voxel stamp_source.  The 48 orientations are the 48 symmetries of the box, orient 0
// the identity.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define VRT_BRUSH_HD __host__ __device__ inline
#else
#define VRT_BRUSH_HD inline
#endif

// (include/vrt.h has the same values for the C-ABI; vrt_api_edit.hip asserts that they agree)
#define VRT_BRUSH_SHAPE_BOX 0
#define VRT_BRUSH_SHAPE_ELLIPSOID 1
#define VRT_BRUSH_SHAPE_CAPSULE 2
#define VRT_BRUSH_MODE_SET 0
#define VRT_BRUSH_MODE_PAINT 1
#define VRT_BRUSH_MODE_ADD 2
#define VRT_BRUSH_MODE_REPLACE 3

#define VRT_BRUSH_MAX_RADIUS 1024       // half voxels
#define VRT_BRUSH_CAPSULE_MIN (-4096)   // a capsule's end points, half voxels
#define VRT_BRUSH_CAPSULE_MAX 12288
#define VRT_BRUSH_BOX_MAX_SIZE (1 << 30)
#define VRT_STAMP_MAX_SIDE 512u
#define VRT_STAMP_ORIENTATIONS 48

namespace vrt {

// floor(v / 2) for either sign
VRT_BRUSH_HD int64_t brush_floor_half(int64_t v) { return v >= 0 ? v / 2 : -((1 - v) / 2); }

// the voxels whose centre 2x+1 lies in [m, M] (half voxels): [*lo, *hi)
VRT_BRUSH_HD void brush_axis_span(int64_t m, int64_t M, int64_t* lo, int64_t* hi)
{
    *lo = brush_floor_half(m);            // ceil((m - 1) / 2)
    *hi = brush_floor_half(M - 1) + 1;
}

// shape and parameters as the predicate wants them; false: unknown shape or a parameter outside its range
VRT_BRUSH_HD bool brush_shape_ok(int32_t shape, const int32_t p[9])
{
    if (shape == VRT_BRUSH_SHAPE_BOX) {
        for (int a = 0; a < 3; a++)
            if (p[3 + a] < 1 || p[3 + a] > VRT_BRUSH_BOX_MAX_SIZE) return false;
        return true;
    }
    if (shape == VRT_BRUSH_SHAPE_ELLIPSOID) {
        for (int a = 0; a < 3; a++)
            if (p[3 + a] < 1 || p[3 + a] > VRT_BRUSH_MAX_RADIUS) return false;
        return true;
    }
    if (shape == VRT_BRUSH_SHAPE_CAPSULE) {
        for (int a = 0; a < 6; a++)
            if (p[a] < VRT_BRUSH_CAPSULE_MIN || p[a] > VRT_BRUSH_CAPSULE_MAX) return false;
        return p[6] >= 1 && p[6] <= VRT_BRUSH_MAX_RADIUS;
    }
    return false;
}

// a mode and the condition it puts on the brush's ids
VRT_BRUSH_HD bool brush_mode_ok(int32_t mode, uint32_t id, uint32_t match)
{
    if (mode == VRT_BRUSH_MODE_SET) return true;
    if (mode == VRT_BRUSH_MODE_PAINT || mode == VRT_BRUSH_MODE_ADD) return id != 0u;
    if (mode == VRT_BRUSH_MODE_REPLACE) return id != match;
    return false;
}

// the voxel box [lo, hi) that holds every voxel the (checked) shape covers, before clipping
VRT_BRUSH_HD void brush_bounds(int32_t shape, const int32_t p[9], int64_t lo[3], int64_t hi[3])
{
    for (int a = 0; a < 3; a++) {
        if (shape == VRT_BRUSH_SHAPE_BOX) { lo[a] = (int64_t)p[a]; hi[a] = (int64_t)p[a] + (int64_t)p[3 + a]; }
        else if (shape == VRT_BRUSH_SHAPE_ELLIPSOID) brush_axis_span((int64_t)p[a] - p[3 + a], (int64_t)p[a] + p[3 + a], &lo[a], &hi[a]);
        else {
            const int64_t m = p[a] < p[3 + a] ? p[a] : p[3 + a], M = p[a] < p[3 + a] ? p[3 + a] : p[a];
            brush_axis_span(m - p[6], M + p[6], &lo[a], &hi[a]);
        }
    }
}

// [lo, hi) cut to the volume -> clo, csize; false: nothing is left
VRT_BRUSH_HD bool brush_clip(const int64_t lo[3], const int64_t hi[3], const int32_t dim[3], int32_t clo[3], uint32_t csize[3])
{
    bool any = true;
    for (int a = 0; a < 3; a++) {
        const int64_t l = lo[a] > 0 ? lo[a] : 0, h = hi[a] < (int64_t)dim[a] ? hi[a] : (int64_t)dim[a];
        clo[a] = h > l ? (int32_t)l : 0;
        csize[a] = h > l ? (uint32_t)(h - l) : 0u;
        any = any && h > l;
    }
    return any;
}

// do the bounds [mn, mx] (max inclusive) that an extent kernel reports lie inside the clipped bounds [clo, clo + csize)?  A record
// nothing touched (mn = INT32_MAX, mx = INT32_MIN) does not.  (Hidden: an out-of-line copy stays out of libvrt_hip.so's dynamic symbols.)
__attribute__((visibility("hidden"))) VRT_BRUSH_HD bool brush_extent_ok(const int32_t mn[3], const int32_t mx[3], const int32_t clo[3], const uint32_t csize[3])
{
    for (int a = 0; a < 3; a++)
        if (mn[a] < clo[a] || mx[a] < mn[a] || (int64_t)mx[a] >= (int64_t)clo[a] + (int64_t)csize[a]) return false;
    return true;
}

// is voxel (x, y, z) inside the (checked) shape?
VRT_BRUSH_HD bool brush_inside(int32_t shape, const int32_t p[9], int32_t x, int32_t y, int32_t z)
{
    const int64_t v[3] = {x, y, z};
    int64_t lo[3], hi[3];
    brush_bounds(shape, p, lo, hi);
    for (int a = 0; a < 3; a++)
        if (v[a] < lo[a] || v[a] >= hi[a]) return false;
    if (shape == VRT_BRUSH_SHAPE_BOX) return true;
    const int64_t P[3] = {2 * v[0] + 1, 2 * v[1] + 1, 2 * v[2] + 1};
    if (shape == VRT_BRUSH_SHAPE_ELLIPSOID) {
        const int64_t dx = P[0] - p[0], dy = P[1] - p[1], dz = P[2] - p[2];
        const int64_t rx2 = (int64_t)p[3] * p[3], ry2 = (int64_t)p[4] * p[4], rz2 = (int64_t)p[5] * p[5];
        return dx * dx * (ry2 * rz2) + dy * dy * (rx2 * rz2) + dz * dz * (rx2 * ry2) <= rx2 * ry2 * rz2;
    }
    int64_t L2 = 0, q = 0, da2 = 0, db2 = 0;
    for (int a = 0; a < 3; a++) {
        const int64_t e = (int64_t)p[3 + a] - p[a], da = P[a] - p[a], db = P[a] - p[3 + a];
        L2 += e * e; q += da * e; da2 += da * da; db2 += db * db;
    }
    const int64_t r2 = (int64_t)p[6] * p[6];
    if (q <= 0 || L2 == 0) return da2 <= r2;
    if (q >= L2) return db2 <= r2;
    return da2 * L2 - q * q <= r2 * L2;
}

// what a voxel inside the shape becomes
VRT_BRUSH_HD uint32_t brush_value(int32_t mode, uint32_t old, uint32_t id, uint32_t match)
{
    if (mode == VRT_BRUSH_MODE_PAINT) return old != 0u ? id : old;
    if (mode == VRT_BRUSH_MODE_ADD) return old == 0u ? id : old;
    if (mode == VRT_BRUSH_MODE_REPLACE) return old == match ? id : old;
    return id;
}

// ---- stamps -------------------------------------------------------------------------------------------------------------------
VRT_BRUSH_HD bool stamp_orient_ok(uint32_t orient) { return orient < 64u && (orient & 7u) < 6u; }

// the source axis that feeds destination axis a
VRT_BRUSH_HD int stamp_perm_axis(uint32_t orient, int a)
{
    const uint32_t perm = orient & 7u;
    // rows of the table above, two bits per destination axis (x lowest)
    const uint32_t code = perm == 0u ? 0x24u : perm == 1u ? 0x18u : perm == 2u ? 0x21u : perm == 3u ? 0x09u : perm == 4u ? 0x12u : 0x06u;
    return (int)((code >> (2 * a)) & 3u);
}

VRT_BRUSH_HD void stamp_dst_size(uint32_t orient, const uint32_t size[3], uint32_t dsize[3])
{
    for (int a = 0; a < 3; a++) dsize[a] = size[stamp_perm_axis(orient, a)];
}

// destination offset (dx, dy, dz) inside the oriented box -> the offset of its source voxel inside the source box
VRT_BRUSH_HD void stamp_source(uint32_t orient, const uint32_t size[3], uint32_t dx, uint32_t dy, uint32_t dz, uint32_t s[3])
{
    const uint32_t d[3] = {dx, dy, dz};
    for (int t = 0; t < 3; t++) {                  // (selects, not s[perm]: every index is a constant once the loops are unrolled)
        uint32_t v = 0u;
        for (int a = 0; a < 3; a++)
            if (stamp_perm_axis(orient, a) == t) v = ((orient >> (3 + a)) & 1u) ? size[t] - 1u - d[a] : d[a];
        s[t] = v;
    }
}

// what a stamped voxel becomes
VRT_BRUSH_HD uint32_t stamp_value(uint32_t old, uint32_t src, bool skip_empty) { return (skip_empty && src == 0u) ? old : src; }

} // namespace vrt
