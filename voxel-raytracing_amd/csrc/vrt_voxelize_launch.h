// vrt_voxelize_launch.h -- what vrt_voxelize.hip's kernels are handed and their launchers, for vrt_voxelize.hip and
// vrt_api_edit.hip (behind <hip/hip_runtime.h>).  vrt_voxelize.h has the definitions and the layout of the masks.
#pragma once

#include "vrt_voxelize.h"
#include "vrt_brush_launch.h"          // BrushRecord, brush_value, and vrt_scene_read.h's ReadBox

namespace vrt {

// One voxelization.  box.lo / box.size say which voxels of the scene a launch runs over: the clipped bounds for k_vox_extent, the
// tight box of the changed voxels for k_vox_compose; box's other members are the scene (ReadBox).  The masks always lie over the
// clipped bounds: clo and csize.
struct VoxJob {
    ReadBox             box;
    int32_t             clo[3];
    uint32_t            csize[3];
    int32_t             mode;
    uint32_t            id, match;
    const int32_t*      vertices;       // device: nv * 3
    const uint32_t*     triangles;      // device: nt * 3
    unsigned long long* cover;          // rows * vox_cover_words(csize[0])
    unsigned long long* toggle;         // rows * vox_toggle_words(csize[0]); NULL without SOLID
};

// What k_vox_extent returns: how many voxels the mesh covers inside the bounds, and the edit (BrushRecord: the covered voxels
// whose id changes).  Sum, min, max and or commute.
struct VoxRecord {
    BrushRecord        edit;
    unsigned long long covered;
};

inline VoxRecord vox_record_init()
{
    VoxRecord r{};
    r.edit = brush_record_init();
    return r;
}

// cover holds zeros (or what an earlier launch of the same call left).  items: device, one wave each; an item's rows are rows of
// its triangle's clipped box (vox_tri_box, solid = false)
hipError_t launch_vox_surface(const VoxJob& j, const VoxItem* items, uint32_t nitems, hipStream_t s);
// toggle holds zeros.  An item's `count` are columns of its triangle's clipped yz-box (vox_tri_box, solid = true), a lane each
hipError_t launch_vox_cross(const VoxJob& j, const VoxItem* items, uint32_t nitems, hipStream_t s);
// the toggle mask's rows scanned and ORed into the coverage mask
hipError_t launch_vox_scan(const VoxJob& j, hipStream_t s);
// rec: device, holding vox_record_init()
hipError_t launch_vox_extent(const VoxJob& j, VoxRecord* rec, hipStream_t s);
// ids: device, box.size[0] * box.size[1] * box.size[2] bytes, read_box_index order: the ids the box holds after the call
hipError_t launch_vox_compose(const VoxJob& j, uint8_t* ids, hipStream_t s);

} // namespace vrt
