// vrt_faces_launch.h -- what vrt_faces.hip's kernels are handed and their launchers, for vrt_faces.hip and vrt_api_faces.hip
// (behind <hip/hip_runtime.h>).  vrt_faces.h has the definitions.
#pragma once

#include "vrt_faces.h"

#if !defined(VRT_SCENE_READ_LAUNCHERS)
#error "define VRT_SCENE_READ_LAUNCHERS ahead of vrt_scene_read.h: the kernels read a box through its ReadBox"
#endif

namespace vrt {

// One extraction: the box and the scene (ReadBox), the volume's size (a neighbour outside it is empty) and the flags.
struct FacesJob {
    ReadBox  box;
    int32_t  dim[3];
    uint32_t flags;
};

// The scan words of a call: the counts of direction d's segments start at faces_work_offset(d), direction-major, so the scan of
// all of them is the output order; faces_work_offset(6) is their number.
inline uint32_t faces_work_offset(const FacesJob& j, uint32_t d)
{
    uint32_t n = 0;
    for (uint32_t k = 0; k < d; k++) n += face_segments(k, j.box.size);
    return n;
}
inline uint32_t faces_work_words(const FacesJob& j) { return faces_work_offset(j, VRT_FACES_DIRECTIONS); }

// work: faces_work_words(j) + 1 + 7 words (device).  After launch_faces_count, work[faces_work_offset(d) + g] is the first record
// of segment g of direction d, work[words] the number of records, and work[words + 1 + d], d = 0 .. 6, the first record of
// direction d (d = 6: the total once more) -- the seven words the host reads.
hipError_t launch_faces_count(const FacesJob& j, uint32_t* work, hipStream_t s);
// writes the `total` records (nothing at or beyond total)
hipError_t launch_faces_scatter(const FacesJob& j, const uint32_t* work, uint32_t total, uint64_t* records, hipStream_t s);

} // namespace vrt
