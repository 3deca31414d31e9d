// vrt_brush_launch.h -- what vrt_brush.hip's kernels are handed and their launchers, for vrt_brush.hip and vrt_api_edit.hip
// (behind <hip/hip_runtime.h>).  vrt_brush.h has the definitions.
#pragma once

#include "vrt_brush.h"
#define VRT_SCENE_READ_LAUNCHERS
#include "vrt_scene_read.h"

namespace vrt {

#define VRT_BRUSH_FORM_STAMP 3        // the kernels' fourth form, after the three shapes

// One brush or stamp.  box.lo / box.size say which voxels of the scene a launch runs over: the clipped bounds for the extent
// kernel, the tight box of the changed voxels for the compose kernel; box's other members are the scene (ReadBox).
struct BrushJob {
    ReadBox        box;
    int32_t        form;          // VRT_BRUSH_SHAPE_* or VRT_BRUSH_FORM_STAMP
    int32_t        mode;
    int32_t        p[9];
    uint32_t       id, match;
    // a stamp: the gathered source box (read_box_index order), where its oriented image lies in the destination, how it is oriented
    const uint8_t* stage;
    int32_t        dst_lo[3];
    uint32_t       src_size[3];
    uint32_t       orient, skip_empty;
};

// What the extent kernel returns: how many voxels change, their bounds (max inclusive) and the set of ids written, bit id of
// word id / 32.  Sum, min, max and or commute: the record does not depend on the schedule.
struct BrushRecord {
    unsigned long long changed;
    int32_t            mn[3], mx[3];
    uint32_t           ids[8];
};

inline BrushRecord brush_record_init()
{
    BrushRecord r{};
    for (int a = 0; a < 3; a++) { r.mn[a] = INT32_MAX; r.mx[a] = INT32_MIN; }
    return r;
}

// rec: device, holding brush_record_init()
hipError_t launch_brush_extent(const BrushJob& j, BrushRecord* rec, hipStream_t s);
// ids: device, box.size[0] * box.size[1] * box.size[2] bytes, read_box_index order: the ids the box holds after the brush
hipError_t launch_brush_compose(const BrushJob& j, uint8_t* ids, hipStream_t s);

} // namespace vrt
