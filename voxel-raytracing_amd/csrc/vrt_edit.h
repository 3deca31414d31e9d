// vrt_edit.h -- which bytes of a dense scene's clearance fields an edit of a box of voxels can change (vrt_scene_edit_box).
// Plain integer arithmetic, compiled for the device (vrt_scene_edit.hip), the host (vrt_api_edit.hip) and the tests
// (tests/native/edit_host.cpp, which checks every statement below against a brute-force rebuild).
//
// Octant o has the signs s = (bit 0: +x, bit 1: +y, bit 2: +z; a clear bit: -).  c_o(p) = min(cap, distance in the octant's
// Chebyshev sense from p to the nearest solid voxel or wall), and an OPEN cell (the whole corner box from p towards s is empty)
// holds the code 0 instead.  For an edit of the box B = [lo, hi):
//   R_o  B grown by cap - 1 AGAINST s on each axis, clipped: the only cells whose clearance can change (a solid further away
//        than cap - 1 is beyond the cap).  Recomputing R_o reads the voxels of
//   E    B grown by cap - 1 on BOTH sides, clipped (R_o grown by cap - 1 towards s; the same box for every octant).
//   Q_o  the corner box from the volume's corner opposite to s up to B's far face in the sense of s: the only cells whose
//        corner box meets B, i.e. whose open state can change.  R_o lies inside Q_o.
// A cell of Q_o that is open after the edit gets 0.  A cell of Q_o outside R_o that WAS open and no longer is held no
// clearance (its byte was the code 0); its corner box was empty and the new solids are beyond its cap, so its clearance is
// edit_wall_clearance(): min(cap, room to the walls towards s, the cell itself counted).  Every other byte keeps its value.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define VRT_EDIT_HD __host__ __device__ inline
#else
#define VRT_EDIT_HD inline
#endif

#define VRT_EDIT_CAP 127          // == VRT_DF_CAP (vrt_device_common.h; vrt_scene_edit.hip asserts it)
#define VRT_EDIT_MAX_SIDE 512     // a longer box side is rebuilt in full: the scan kernels hold a line of side + 2 (cap - 1) in LDS

namespace vrt {

struct EditSpan { int lo, hi; };     // [lo, hi)

VRT_EDIT_HD int edit_min(int a, int b) { return a < b ? a : b; }
VRT_EDIT_HD int edit_max(int a, int b) { return a > b ? a : b; }

// one axis of R_o: sign > 0 grows towards lower coordinates
VRT_EDIT_HD EditSpan edit_span_r(int lo, int hi, int dim, int sign, int cap)
{
    EditSpan r;
    r.lo = sign > 0 ? edit_max(0, lo - (cap - 1)) : lo;
    r.hi = sign > 0 ? hi : edit_min(dim, hi + (cap - 1));
    return r;
}
// one axis of E
VRT_EDIT_HD EditSpan edit_span_e(int lo, int hi, int dim, int cap)
{
    EditSpan r;
    r.lo = edit_max(0, lo - (cap - 1));
    r.hi = edit_min(dim, hi + (cap - 1));
    return r;
}
// one axis of Q_o
VRT_EDIT_HD EditSpan edit_span_q(int lo, int hi, int dim, int sign)
{
    EditSpan r;
    r.lo = sign > 0 ? 0 : lo;
    r.hi = sign > 0 ? hi : dim;
    return r;
}
// clearance of a cell whose whole corner box towards the signs (sx, sy, sz) is empty
VRT_EDIT_HD int edit_wall_clearance(int x, int y, int z, int W, int H, int D, int sx, int sy, int sz, int cap)
{
    const int rx = sx > 0 ? W - x : x + 1, ry = sy > 0 ? H - y : y + 1, rz = sz > 0 ? D - z : z + 1;
    return edit_min(cap, edit_min(rx, edit_min(ry, rz)));
}
// The rule of vrt_scene_edit_box: an edit is done in place while the cells to recompute, summed over the octants, are fewer
// than half of what a full build computes (8 W H D) and no side of the box exceeds VRT_EDIT_MAX_SIDE; else the fields are
// rebuilt in full (the result is the same either way).
VRT_EDIT_HD bool edit_in_place(int W, int H, int D, const int lo[3], const int hi[3], int cap)
{
    const int dim[3] = {W, H, D};
    uint64_t sum = 0;
    for (int o = 0; o < 8; o++) {
        uint64_t n = 1;
        for (int a = 0; a < 3; a++) {
            const EditSpan r = edit_span_r(lo[a], hi[a], dim[a], ((o >> a) & 1) ? 1 : -1, cap);
            n *= (uint64_t)(r.hi - r.lo);
        }
        sum += n;
    }
    for (int a = 0; a < 3; a++)
        if (hi[a] - lo[a] > VRT_EDIT_MAX_SIDE) return false;
    return sum < 4ull * (uint64_t)W * (uint64_t)H * (uint64_t)D;
}

} // namespace vrt
