// vrt_morph_launch.h -- what vrt_morph.hip's kernels are handed and their launchers, for vrt_morph.hip and vrt_api_edit.hip
// (behind <hip/hip_runtime.h>).  vrt_morph.h has the definitions, the layout of the masks and the argument that a tile is exact.
#pragma once

#include "vrt_morph.h"
#include "vrt_brush_launch.h"          // BrushRecord, and vrt_scene_read.h's ReadBox

namespace vrt {

// One operation.  box.lo / box.size say which voxels of the scene a launch runs over: the clipped bounds for k_morph_extent, the
// tight box of the changed voxels for k_morph_compose; box's other members are the scene (ReadBox).  The masks always lie over
// the domain: mlo and msize.
struct MorphJob {
    ReadBox         box;
    int32_t         dim[3];      // the volume's sides: a cell of the domain outside them is the border's
    int32_t         mlo[3];      // the domain's low corner (the clipped bounds' less the halo; may be negative)
    uint32_t        msize[3];    // the domain's sides
    int32_t         op, connectivity;
    uint32_t        radius, border_solid, id;
    uint32_t*       mask[2];     // morph_mask_words(msize) words each: A (the mask pass writes it) and B
    const uint32_t* result;      // mask[1] after one phase, mask[0] after two: what the extent and compose kernels read
};

// What k_morph_extent returns: the edit (BrushRecord) and how many of its voxels were added and removed.  Sum, min, max and or commute.
struct MorphRecord {
    BrushRecord        edit;
    unsigned long long added, removed;
};

inline MorphRecord morph_record_init()
{
    MorphRecord r{};
    r.edit = brush_record_init();
    return r;
}

// S over the domain into mask[0]
hipError_t launch_morph_pass(const MorphJob& j, hipStream_t s);
// one phase: dil_r (erode: ero_r) of src into dst, both over the domain
hipError_t launch_morph_step(const MorphJob& j, const uint32_t* src, uint32_t* dst, bool erode, hipStream_t s);
// rec: device, holding morph_record_init()
hipError_t launch_morph_extent(const MorphJob& j, MorphRecord* rec, hipStream_t s);
// ids: device, box.size[0] * box.size[1] * box.size[2] bytes, read_box_index order: the ids the box holds after the operation
hipError_t launch_morph_compose(const MorphJob& j, uint8_t* ids, hipStream_t s);

} // namespace vrt
