// vrt_brick_edit.h -- which bytes of a brick scene an edit of a box of voxels can change (vrt_scene_edit_box on a scene that
// vrt_scene_reserve_bricks made editable).  Plain integer arithmetic, compiled for the device (vrt_scene_edit.hip), the host
// (vrt_api_edit.hip) and the tests (tests/native/brick_edit_host.cpp, which checks every statement below against a brute-force build).
//
// The volume is a lattice of 8^3 bricks.  For an edit of the voxel box B = [lo, hi):
//   T    the bricks B meets: the only bricks whose ids, pool slot and occupancy can change.
//   F    T grown by one brick on every side, clipped: the only bricks whose per-voxel clearance (bfine) can change -- a brick's
//        fine bytes are a function of the voxels of its 3 x 3 x 3 brick neighbourhood (k_brick_fine), and the cap of 16 voxels
//        reaches no further.  Only the bricks of F that are occupied after the edit hold fine bytes, so only those are recomputed.
// If no brick of T changed its OCCUPANCY, that is all: the coarse fields, the open bits, the packed entries and the cell list
// are functions of the bricks' occupancy and of their pool slots, and neither changed.  Otherwise the coarse fields are the dense
// scene's clearance transform over the brick lattice with cap 16 (vrt_edit.h with T in the place of B):
//   R_o  T grown by 15 bricks AGAINST the octant's signs, clipped: the only bricks whose coarse clearance can change.
//        Recomputing R_o reads the occupancy of
//   E    T grown by 15 bricks on BOTH sides, clipped.  A transform of the sub-lattice E alone, its outside counted as solid, gives
//        the right value at every brick of R_o: where E was clipped the outside IS solid (the volume's wall), and elsewhere a
//        look-up that starts in R_o and runs towards the signs ends, at 15 bricks, inside E.
//   Q_o  the corner box from the volume's corner opposite to the signs up to T's far face: the only bricks whose corner box
//        meets T, i.e. whose open state can change.  The open flag is bit 7 BESIDE the clearance (not the code 0 of the dense
//        fields), so a brick that stops being open needs no clearance reconstructed: its low seven bits are already right.
// Every other byte keeps its value.
#pragma once

#include "vrt_edit.h"

#define VRT_BRICK_EDIT_CAP 16     // the cap of the coarse fields (vrt_scene_from_bricks builds them with launch_build_df(..., 16))

namespace vrt {

// one axis of T: the bricks the voxel span [lo, hi) meets
VRT_EDIT_HD EditSpan brick_span_t(int lo, int hi)
{
    EditSpan r;
    r.lo = lo >> 3;
    r.hi = ((hi - 1) >> 3) + 1;
    return r;
}
// one axis of F, from the same axis of T; nb: bricks along the axis
VRT_EDIT_HD EditSpan brick_span_f(EditSpan t, int nb)
{
    EditSpan r;
    r.lo = edit_max(0, t.lo - 1);
    r.hi = edit_min(nb, t.hi + 1);
    return r;
}
// one axis of R_o, E and Q_o, from the same axis of T
VRT_EDIT_HD EditSpan brick_span_r(EditSpan t, int nb, int sign) { return edit_span_r(t.lo, t.hi, nb, sign, VRT_BRICK_EDIT_CAP); }
VRT_EDIT_HD EditSpan brick_span_e(EditSpan t, int nb) { return edit_span_e(t.lo, t.hi, nb, VRT_BRICK_EDIT_CAP); }
VRT_EDIT_HD EditSpan brick_span_q(EditSpan t, int nb, int sign) { return edit_span_q(t.lo, t.hi, nb, sign); }

// The rule of an edit that CHANGED some brick's occupancy (lo, hi: the voxel box): the coarse fields are updated in place while
// the bricks to recompute, summed over the octants, are fewer than half of what a full build computes (8 nbx nby nbz) -- the
// share vrt_edit.h takes; else the edit goes through the full build path: the coarse fields, the open bits and the fine bytes of
// EVERY occupied brick are built again (the result is the same either way).  An edit that changed no brick's occupancy recomputes
// the occupied bricks of F and nothing else, which is never more than the full build's fine pass, and is always done in place.
VRT_EDIT_HD bool brick_edit_in_place(int nbx, int nby, int nbz, const int lo[3], const int hi[3])
{
    const int nb[3] = {nbx, nby, nbz};
    uint64_t sum = 0;
    for (int o = 0; o < 8; o++) {
        uint64_t n = 1;
        for (int a = 0; a < 3; a++) {
            const EditSpan r = brick_span_r(brick_span_t(lo[a], hi[a]), nb[a], ((o >> a) & 1) ? 1 : -1);
            n *= (uint64_t)(r.hi - r.lo);
        }
        sum += n;
    }
    return sum < 4ull * (uint64_t)nbx * (uint64_t)nby * (uint64_t)nbz;
}

} // namespace vrt
