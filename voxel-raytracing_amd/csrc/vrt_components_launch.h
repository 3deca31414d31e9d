// vrt_components_launch.h -- what vrt_components.hip's kernels are handed and their launchers, for vrt_components.hip and
// vrt_api_components.hip (behind <hip/hip_runtime.h>).  vrt_components.h has the definition, the passes and their argument.
#pragma once

#include "vrt_components.h"
#include "vrt_brush_launch.h"          // BrushRecord, and vrt_scene_read.h's ReadBox and segments

namespace vrt {

// One labelling.  box.lo / box.size say which voxels of the scene a launch runs over: the clipped bounds for every pass and
// k_comp_extent, the tight box of the changed voxels for k_comp_compose; box's other members are the scene (ReadBox).  The
// label volume always lies over the clipped bounds: clo, csize and nt.
struct CompJob {
    ReadBox   box;
    int32_t   clo[3];
    uint32_t  csize[3];
    uint32_t  nt[3];             // tiles per axis
    int32_t   match, connectivity;
    uint32_t  id;                // the filter's
    uint32_t* labels;            // csize[0] * csize[1] * csize[2] words
    CompStat* table;             // ncomp entries (passes 4 and later)
    uint32_t  ncomp;
};

// What k_comp_summary and k_comp_select return.  Max and sums commute.
struct CompSummary {
    unsigned long long largest;              // comp_largest_key of the largest component; 0: there is none
    unsigned long long voxels;               // passing voxels
    unsigned long long sel_components, sel_voxels;
};

// What k_comp_extent returns: the edit (BrushRecord: the voxels of selected components whose id differs from the filter's)
struct CompFilter { unsigned long long min_voxels, max_voxels; uint32_t faces_all, faces_none, flags, largest; };

// passes 1 to 3 (vrt_components.h); work: list_segments(j.box) + 1 words, after launch_comp_flatten the roots of every segment
hipError_t launch_comp_tile(const CompJob& j, hipStream_t s);
hipError_t launch_comp_seam(const CompJob& j, hipStream_t s);
hipError_t launch_comp_flatten(const CompJob& j, uint32_t* work, hipStream_t s);
// passes 4 to 6; work holds the scanned counts (launch_list_scan), j.table room for j.ncomp = work[segments] entries;
// sum: device, holding zeros
hipError_t launch_comp_number(const CompJob& j, const uint32_t* work, hipStream_t s);
hipError_t launch_comp_measure(const CompJob& j, hipStream_t s);
hipError_t launch_comp_summary(const CompJob& j, CompSummary* sum, hipStream_t s);
// the filter: marks the selected entries of the table and counts them into sum (sel_components and sel_voxels hold zeros)
hipError_t launch_comp_select(const CompJob& j, const CompFilter& f, CompSummary* sum, hipStream_t s);
// rec: device, holding brush_record_init()
hipError_t launch_comp_extent(const CompJob& j, BrushRecord* rec, hipStream_t s);
// ids: device, box.size[0] * box.size[1] * box.size[2] bytes, read_box_index order: the ids the box holds after the filter
hipError_t launch_comp_compose(const CompJob& j, uint8_t* ids, hipStream_t s);
// out: device, size[0] * size[1] * size[2] words, read_box_index order: the labels of the box [lo, lo + size) inside the clipped bounds
hipError_t launch_comp_labels(const CompJob& j, const int32_t lo[3], const uint32_t size[3], uint32_t* out, hipStream_t s);

} // namespace vrt
