// vrt_traverse.h -- the grid march of voxel_volume.frag:109-174 (boxIntersection + traceRayInt) in traversal strategies
// that all produce the SAME RayInt (hit cell, mask, sideDist, material) bit for bit:
//
//   DENSE    one R8 fetch per DDA iteration (the literal shader loop)
//   BITMASK  same iterations; the solid test reads the 4^3 occupancy word cached in registers and the
//            16^3 summary (LDS) before touching global memory; the R8 id is fetched once, at the hit
//   DF       the wave agrees (one DPP min-reduction) on a number of iterations no lane needs a memory test for (distance
//            field clearance) and runs them as pure ALU stepping; one gather per run instead of per iteration
//   DF_FAST  DF through four hand-written gfx950 look-up loops (what AUTO / DF resolve to; _CNT: their counting twins)
//   BRICK    DF over the two-level clearance of a brick scene (_CNT: with its counters)
//   JUMP     BITMASK inside occupied 4^3 cells; across EMPTY pyramid cells (4^3 / 16^3 / 64^3) one iteration
//            replaces all the DDA iterations up to the cell's exit -- exactly (see "exact jumps" further down)
//   DFJ      DF with its long runs in that closed form
//
// Compiled for the device by vrt_device.hip and vrt_query.hip and for the host by tests/native/traverse_host.cpp (unit tests
// of this very code against the oracle on millions of rays; the shipped library has no host render path).
//
// The data types and the DDA are in vrt_volume.h and vrt_dda.h (no march, no assembly: what the C-ABI and the scene build
// include).  One header per march, included here in this order: vrt_march_df.h (DF in plain C++: trace_df),
// vrt_march_fast.h (the hand-written loops: trace_df_fast, the AO pool), vrt_march_brick.h (the brick march and its pool),
// vrt_march_literal.h (DENSE, BITMASK, the exact jumps: trace_jump, trace_dfj); each ends with the host stubs of its own
// device-only functions.  This file holds trace_int, the dispatch.
#pragma once

#include "vrt_dda.h"     // (over vrt_volume.h: the data types and the DDA, for code that needs no march)
#include "vrt_march_df.h"
#include "vrt_march_fast.h"
#include "vrt_march_brick.h"
#include "vrt_march_literal.h"

namespace vrt {

// Dispatcher used by the kernels.
// ANYHIT: the caller only uses r.material and r.fetches (traceRayHit, frag:198-202): a traversal may then stop stepping a ray
// that is certain to exhaust its budget in empty space (DF_FAST does)
template <int TRAV, class OP, bool AHEAD = false, bool ANYHIT = false, bool PF = false, bool OWN = false>
VRT_HD void trace_int(const VolumeView& v, OP o2, OP o3, f3 start, f3 dir,
                      uint32_t maxSteps, RayInt& r)
{
    if (TRAV == VRT_TRAVERSAL_JUMP) {
        NoStats ns;
        trace_jump(v, o2, o3, start, dir, maxSteps, r, ns);
    } else if (TRAV == VRT_TRAVERSAL_BRICK) {
        NoStats ns;
        if (ANYHIT && OWN && v.df_own) trace_brick_own(v, start, dir, maxSteps, r, ns);
        else trace_brick<NoStats, ANYHIT>(v, start, dir, maxSteps, r, ns);
    } else if (TRAV == VRT_TRAVERSAL_BRICK_CNT) {
        NoStats ns;
        if (ANYHIT && OWN && v.df_own) trace_brick_own<NoStats, true>(v, start, dir, maxSteps, r, ns);
        else trace_brick<NoStats, ANYHIT, true>(v, start, dir, maxSteps, r, ns);
    } else if (TRAV == VRT_TRAVERSAL_DF_FAST) {
        NoStats ns;
        trace_df_fast<NoStats, ANYHIT, PF, OWN>(v, start, dir, maxSteps, r, ns);
    } else if (TRAV == VRT_TRAVERSAL_DF_FAST_CNT) {
        NoStats ns;
        trace_df_fast<NoStats, ANYHIT, PF, OWN, true>(v, start, dir, maxSteps, r, ns);
    } else if (TRAV == VRT_TRAVERSAL_DF) {
        NoStats ns;
        trace_df<NoStats, AHEAD>(v, start, dir, maxSteps, r, ns);
    } else if (TRAV == VRT_TRAVERSAL_DFJ) {
        NoStats ns;
        trace_dfj(v, start, dir, maxSteps, r, ns);
    } else {
        trace_literal<TRAV>(v, o2, start, dir, maxSteps, r);
    }
}

} // namespace vrt
