// vrt_faces.hip -- surface extraction kernels for gfx950 (vrt_scene_list_faces) and their launchers.  vrt_faces.h has the
// definitions: exposed faces, runs, the record, the order, and why the listing needs no sort.
//   k_faces_count<BRICK, YROWS>    one wave per segment of 64 voxels along the run axis: per direction the ballot of "exposed" and
//                                  of "continues the lane below", the population count of the run starts into the scan words
//   k_faces_totals                 behind the scan (vrt_scene_read.hip's k_list_scan): the seven words the host reads
//   k_faces_scatter<BRICK, YROWS>  the same ballots again; a start's record goes to its segment's first record + the starts below
// YROWS = true takes d = 0, 1 (-x, +x), whose runs lie along y: lane l of a segment holds (bx, 64 s + l, bz), so a wave's 64 loads
// of the ids are W bytes apart (bricks: 8 bytes apart within a brick) and consecutive segments are consecutive bx -- the four
// waves of a block and the blocks beside it read the same lines.  YROWS = false takes d = 2 .. 5, whose runs lie along x as
// vrt_scene_list_box's rows do.  Either way the neighbour across a face is never along the lane axis: it is one more load per
// lane and direction, made by the lanes whose own voxel is non-empty; the lane below (same id, exposed too) comes from a lane shift
// and the ballot.  A call reads the box's own ids four times (count and scatter, each in both layouts) and a non-empty voxel's
// six neighbours twice.  An empty brick costs the 32-bit load of its entry's low half, as in vrt_scene_read.hip.
#include "vrt_device_common.h"
#define VRT_SCENE_READ_LAUNCHERS
#include "vrt_faces_launch.h"

namespace vrt {

// the run starts of one direction of one segment, and the lanes that continue the lane below
struct FaceMasks { uint64_t starts, continues; };

template <bool BRICK>
__device__ __forceinline__ FaceMasks faces_masks(const FacesJob& J, uint32_t d, uint32_t lane, uint32_t bx, uint32_t by, uint32_t bz, uint32_t id,
                                                 uint32_t id_below)
{
    bool exposed = false;
    if (id != 0u) {
        const int32_t b[3] = {(int32_t)bx, (int32_t)by, (int32_t)bz};
        int32_t p[3];
        exposed = !face_neighbour_reads(d, b, J.box.lo, J.box.size, J.dim, J.flags, p) || read_voxel<BRICK>(J.box, p[0], p[1], p[2]) == 0u;
    }
    const uint64_t e = __ballot(exposed);
    uint64_t c = 0;
    if (J.flags & VRT_FACES_FLAG_RUNS)                              // (wave-uniform)
        c = __ballot(exposed && lane != 0u && id_below == id && ((e >> ((lane - 1u) & 63u)) & 1ull) != 0ull);
    return FaceMasks{e & ~c, c};
}

// segment g of the layout -> this lane's voxel and its id (0 beyond the row's end), and the id of the lane below
template <bool BRICK, bool YROWS>
__device__ __forceinline__ void faces_lane(const FacesJob& J, uint32_t g, uint32_t lane, uint32_t& bx, uint32_t& by, uint32_t& bz, uint32_t& id,
                                           uint32_t& id_below)
{
    const bool in_row = face_segment_voxel(YROWS ? 0u : 2u, g, lane, J.box.size, &bx, &by, &bz);
    id = in_row ? read_voxel<BRICK>(J.box, J.box.lo[0] + (int)bx, J.box.lo[1] + (int)by, J.box.lo[2] + (int)bz) : 0u;
    id_below = (uint32_t)__shfl_up((int)id, 1);
}

// four waves per block, a segment each; base: the scan word of segment 0 of the layout's first direction, nseg: its segments
template <bool BRICK, bool YROWS>
__global__ __launch_bounds__(256) void k_faces_count(const FacesJob J, uint32_t base, uint32_t nseg, uint32_t* __restrict__ work)
{
    const uint32_t lane = threadIdx.x & 63u, g = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (g >= nseg) return;                                          // (wave-uniform)
    uint32_t bx, by, bz, id, id_below;
    faces_lane<BRICK, YROWS>(J, g, lane, bx, by, bz, id, id_below);
#pragma unroll
    for (uint32_t k = 0; k < (YROWS ? 2u : 4u); k++) {
        const FaceMasks m = faces_masks<BRICK>(J, (YROWS ? 0u : 2u) + k, lane, bx, by, bz, id, id_below);
        if (lane == 0u) work[base + k * nseg + g] = (uint32_t)__popcll(m.starts);
    }
}

struct FaceOffsets { uint32_t at[VRT_FACES_DIRECTIONS + 1u]; };     // faces_work_offset(d), d = 0 .. 6

__global__ __launch_bounds__(64) void k_faces_totals(uint32_t* __restrict__ work, const FaceOffsets off)
{
    if (threadIdx.x <= VRT_FACES_DIRECTIONS) work[off.at[VRT_FACES_DIRECTIONS] + 1u + threadIdx.x] = work[off.at[threadIdx.x]];
}

template <bool BRICK, bool YROWS>
__global__ __launch_bounds__(256) void k_faces_scatter(const FacesJob J, uint32_t base, uint32_t nseg, const uint32_t* __restrict__ work, uint32_t total,
                                                       uint64_t* __restrict__ records)
{
    const uint32_t lane = threadIdx.x & 63u, g = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (g >= nseg) return;
    uint32_t bx, by, bz, id, id_below;
    faces_lane<BRICK, YROWS>(J, g, lane, bx, by, bz, id, id_below);
#pragma unroll
    for (uint32_t k = 0; k < (YROWS ? 2u : 4u); k++) {
        const uint32_t d = (YROWS ? 0u : 2u) + k;
        const FaceMasks m = faces_masks<BRICK>(J, d, lane, bx, by, bz, id, id_below);
        if (((m.starts >> lane) & 1ull) != 0ull) {
            const uint32_t at = work[base + k * nseg + g] + (uint32_t)__popcll(m.starts & ((1ull << lane) - 1ull));
            // the lanes above that continue, one after the other: the trailing ones of continues >> (lane + 1) (bit 63 of it is 0)
            const uint32_t length = 1u + (uint32_t)__builtin_ctzll(~((m.continues >> 1) >> lane));
            if (at < total) records[at] = face_record(bx, by, bz, id, length, d);
        }
    }
}

template <bool YROWS>
static void faces_layout(const FacesJob& j, uint32_t* base, uint32_t* nseg)
{
    *base = faces_work_offset(j, YROWS ? 0u : 2u);
    *nseg = face_segments(YROWS ? 0u : 2u, j.box.size);
}

hipError_t launch_faces_count(const FacesJob& j, uint32_t* work, hipStream_t s)
{
    uint32_t base, nseg;
    faces_layout<true>(j, &base, &nseg);
    if (j.box.vox) hipLaunchKernelGGL((k_faces_count<false, true>), dim3((nseg + 3u) / 4u), dim3(256), 0, s, j, base, nseg, work);
    else           hipLaunchKernelGGL((k_faces_count<true, true>), dim3((nseg + 3u) / 4u), dim3(256), 0, s, j, base, nseg, work);
    faces_layout<false>(j, &base, &nseg);
    if (j.box.vox) hipLaunchKernelGGL((k_faces_count<false, false>), dim3((nseg + 3u) / 4u), dim3(256), 0, s, j, base, nseg, work);
    else           hipLaunchKernelGGL((k_faces_count<true, false>), dim3((nseg + 3u) / 4u), dim3(256), 0, s, j, base, nseg, work);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if ((e = launch_list_scan(work, faces_work_words(j), s)) != hipSuccess) return e;
    FaceOffsets off;
    for (uint32_t d = 0; d <= VRT_FACES_DIRECTIONS; d++) off.at[d] = faces_work_offset(j, d);
    hipLaunchKernelGGL(k_faces_totals, dim3(1), dim3(64), 0, s, work, off);
    return hipGetLastError();
}

hipError_t launch_faces_scatter(const FacesJob& j, const uint32_t* work, uint32_t total, uint64_t* records, hipStream_t s)
{
    uint32_t base, nseg;
    faces_layout<true>(j, &base, &nseg);
    if (j.box.vox) hipLaunchKernelGGL((k_faces_scatter<false, true>), dim3((nseg + 3u) / 4u), dim3(256), 0, s, j, base, nseg, work, total, records);
    else           hipLaunchKernelGGL((k_faces_scatter<true, true>), dim3((nseg + 3u) / 4u), dim3(256), 0, s, j, base, nseg, work, total, records);
    faces_layout<false>(j, &base, &nseg);
    if (j.box.vox) hipLaunchKernelGGL((k_faces_scatter<false, false>), dim3((nseg + 3u) / 4u), dim3(256), 0, s, j, base, nseg, work, total, records);
    else           hipLaunchKernelGGL((k_faces_scatter<true, false>), dim3((nseg + 3u) / 4u), dim3(256), 0, s, j, base, nseg, work, total, records);
    return hipGetLastError();
}

} // namespace vrt
