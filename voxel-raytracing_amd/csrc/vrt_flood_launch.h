// vrt_flood_launch.h -- what vrt_flood.hip's kernels are handed and their launchers, for vrt_flood.hip and vrt_api_edit.hip
// (behind <hip/hip_runtime.h>).  vrt_flood.h has the definitions, the layout of the masks and the wake-up invariant.
#pragma once

#include "vrt_flood.h"
#include "vrt_brush_launch.h"          // BrushRecord, and vrt_scene_read.h's ReadBox

namespace vrt {

// One flood.  box.lo / box.size say which voxels of the scene a launch runs over: the clipped bounds for k_flood_pass and
// k_flood_extent, the tight box of the changed voxels for k_flood_compose; box's other members are the scene (ReadBox).  The
// masks always lie over the clipped bounds: clo and nt.
struct FloodJob {
    ReadBox  box;
    int32_t  clo[3];             // the clipped bounds' low corner: where the tiles are counted from
    uint32_t nt[3];              // tiles per axis
    int32_t  seed[3];            // inside the clipped bounds
    int32_t  match, connectivity;
    uint32_t id;
    uint8_t* passable;           // flood_tile_count(nt) * 64 bytes each
    uint8_t* reached;
};

// What k_flood_extent returns: the region (its voxels, its bounds, max inclusive), the id found at the seed, and the edit
// (BrushRecord: the voxels of the region whose id differs from the flood's).  Sum, min, max and or commute.
struct FloodRecord {
    BrushRecord        edit;
    unsigned long long region;
    int32_t            mn[3], mx[3];
    uint32_t           seed_id;
};

inline FloodRecord flood_record_init()
{
    FloodRecord r{};
    r.edit = brush_record_init();
    for (int a = 0; a < 3; a++) { r.mn[a] = INT32_MAX; r.mx[a] = INT32_MIN; }
    return r;
}

// passable, reached and act0 hold zeros.  Fills the passable mask, sets the seed's bit of the reached mask and round 0's flags
// in act0 (flood_seed_tiles) if the seed passes, and writes rec->seed_id.
hipError_t launch_flood_pass(const FloodJob& j, uint32_t* act0, FloodRecord* rec, hipStream_t s);
// One round: a step on every tile whose flag in act_cur is set (the flag is cleared), flags for the next round into act_next,
// *marked = 1 if any was set.  prev (may be NULL): the round before's `marked`; a round whose predecessor marked nothing exits.
hipError_t launch_flood_round(const FloodJob& j, uint32_t* act_cur, uint32_t* act_next, const uint32_t* prev, uint32_t* marked, hipStream_t s);
// rec: device, holding flood_record_init() but for seed_id
hipError_t launch_flood_extent(const FloodJob& j, FloodRecord* rec, hipStream_t s);
// ids: device, box.size[0] * box.size[1] * box.size[2] bytes, read_box_index order: the ids the box holds after the flood
hipError_t launch_flood_compose(const FloodJob& j, uint8_t* ids, hipStream_t s);

} // namespace vrt
