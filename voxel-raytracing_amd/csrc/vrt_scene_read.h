// vrt_scene_read.h -- the read half of scene I/O (vrt_scene_read_box, vrt_scene_list_box, the .vox writer): the record a listed
// voxel becomes, the order of the records, the checks of a box and the tiling of a saved scene.  Plain integer arithmetic,
// compiled for the device (vrt_scene_read.hip), the host (vrt_api_scene.hip, vox_writer.cpp) and the tests
// (tests/native/scene_read_host.cpp, which is held against a numpy restatement).
//
// A box is [lo, lo + size) in voxels.  Voxel (x, y, z) of it has the BOX INDEX
//     i = (x - lo[0]) + (y - lo[1]) * size[0] + (z - lo[2]) * size[0] * size[1]                 (x fastest; read_box_index)
// which is where vrt_scene_read_box puts its id, and the order in which vrt_scene_list_box lists the non-empty voxels (id != 0):
// ascending i.  A listed voxel is ONE word,
//     (x - lo[0]) | (y - lo[1]) << 8 | (z - lo[2]) << 16 | id << 24                             (list_record)
// which is why a listed box has no side above VRT_LIST_MAX_SIDE = 256.  The order is part of the contract: the records, and
// the file written from them, are a function of the scene's content alone.  The kernels keep it without sorting: a row of the
// box is cut into SEGMENTS of 64 consecutive x (list_segments_per_row of them; the last may be short), segment
//     g = (x - lo[0]) / 64 + ((y - lo[1]) + (z - lo[2]) * size[1]) * list_segments_per_row(size[0])   (list_segment)
// so ascending g, and ascending lane within a segment, is ascending i.  One wave takes a segment: a ballot of id != 0 gives the
// segment's count and each lane's rank among the lanes below it, an exclusive scan over the segments' counts gives every
// segment's first record.
//
// A saved scene (vox_writer.cpp) is cut into TILES of at most 256 voxels per axis, the last tile of an axis taking the
// remainder (save_tiles / save_tile_span), ordered x fastest, then y, then z; a tile's records are vrt_scene_list_box's of the
// tile's box.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define VRT_READ_HD __host__ __device__ inline
#else
#define VRT_READ_HD inline
#endif

#define VRT_LIST_MAX_SIDE 256u    // a coordinate within a listed box is one byte of the record
#define VRT_LIST_SEGMENT 64u      // voxels of a row one wave ballots
#define VRT_SAVE_TILE 256u        // a .vox model's largest side (its XYZI coordinates are bytes)

namespace vrt {

VRT_READ_HD size_t read_box_index(uint32_t bx, uint32_t by, uint32_t bz, const uint32_t size[3])
{
    return (size_t)bx + ((size_t)by + (size_t)bz * (size_t)size[1]) * (size_t)size[0];
}

VRT_READ_HD uint32_t list_record(uint32_t bx, uint32_t by, uint32_t bz, uint32_t id)
{
    return bx | (by << 8) | (bz << 16) | (id << 24);
}

VRT_READ_HD uint32_t list_segments_per_row(uint32_t size_x) { return (size_x + VRT_LIST_SEGMENT - 1u) / VRT_LIST_SEGMENT; }

VRT_READ_HD uint32_t list_segment(uint32_t bx, uint32_t by, uint32_t bz, const uint32_t size[3])
{
    return bx / VRT_LIST_SEGMENT + (by + bz * size[1]) * list_segments_per_row(size[0]);
}

// What vrt_scene_read_box / vrt_scene_list_box make of a box before any device work (max_side == 0: no limit on the sides)
enum ReadBoxCheck { READ_BOX_OK = 0, READ_BOX_EMPTY = 1, READ_BOX_OVERFLOW = 2, READ_BOX_SIDE = 3, READ_BOX_OUTSIDE = 4 };

VRT_READ_HD ReadBoxCheck read_box_check(const int32_t dim[3], const int32_t lo[3], const uint32_t size[3], uint32_t max_side, size_t* count)
{
    for (int a = 0; a < 3; a++)
        if (size[a] == 0u) return READ_BOX_EMPTY;
    // size[0] * size[1] * size[2] in size_t, with the overflow seen (three 32-bit sides can reach 2^96)
    const size_t top = ~(size_t)0;
    size_t n = (size_t)size[0];
    for (int a = 1; a < 3; a++) {
        if ((size_t)size[a] > top / n) return READ_BOX_OVERFLOW;
        n *= (size_t)size[a];
    }
    for (int a = 0; a < 3; a++)
        if (max_side != 0u && size[a] > max_side) return READ_BOX_SIDE;
    for (int a = 0; a < 3; a++)
        if (lo[a] < 0 || lo[a] >= dim[a] || (uint64_t)size[a] > (uint64_t)(dim[a] - lo[a])) return READ_BOX_OUTSIDE;
    *count = n;
    return READ_BOX_OK;
}

// tiles of a saved scene along an axis of `dim` voxels, and tile t's [lo, lo + size)
VRT_READ_HD uint32_t save_tiles(uint32_t dim) { return (dim + VRT_SAVE_TILE - 1u) / VRT_SAVE_TILE; }
VRT_READ_HD void save_tile_span(uint32_t dim, uint32_t t, uint32_t* lo, uint32_t* size)
{
    *lo = t * VRT_SAVE_TILE;
    *size = dim - *lo < VRT_SAVE_TILE ? dim - *lo : VRT_SAVE_TILE;
}

#if defined(VRT_SCENE_READ_LAUNCHERS)
// ---- the kernels' side and their launchers: for vrt_scene_read.hip and vrt_api_scene.hip, which define VRT_SCENE_READ_LAUNCHERS
// behind <hip/hip_runtime.h> ----------------------------------------------------------------------------------------------
// What a kernel reads a box from: a dense scene's ids (vox) or a brick scene's packed entries and pool (vox == nullptr).
struct ReadBox {
    const uint8_t*  vox;         // dense: W * H * D ids, x + y*W + z*W*H
    const uint64_t* bentry;      // bricks: one word per brick of the padded grid, the pointer in its low 24 bits (VolumeView::bentry)
    const uint8_t*  bpool;       // bricks: 512 ids per pool slot
    uint32_t        bcap;        // bricks: slots the pool has room for (a pointer beyond it reads as an empty brick)
    int32_t         W, H, pbx, pby;
    int32_t         lo[3];
    uint32_t        size[3];
};
// the id of volume voxel (x, y, z), which lies inside the volume
template <bool BRICK>
__device__ __forceinline__ uint32_t read_voxel(const ReadBox& B, int x, int y, int z)
{
    if (!BRICK) return B.vox[(size_t)x + ((size_t)y + (size_t)z * (size_t)B.H) * (size_t)B.W];
    const size_t pc = (size_t)((x >> 3) + 1) + ((size_t)((y >> 3) + 1) + (size_t)((z >> 3) + 1) * (size_t)B.pby) * (size_t)B.pbx;
    const uint32_t ptr = ((const uint32_t*)B.bentry)[2u * pc] & 0xFFFFFFu;          // the entry's low word: pointer | open bits << 24
    if (ptr == 0u || ptr > B.bcap) return 0u;                                      // empty (a border entry, 0xFFFFFF, cannot lie under a box inside the volume)
    return B.bpool[(size_t)(ptr - 1u) * 512u + (size_t)((x & 7) | ((y & 7) << 3) | ((z & 7) << 6))];
}
// ids[read_box_index] of every voxel of the box (device memory, size[0] * size[1] * size[2] bytes)
hipError_t launch_read_box(const ReadBox& b, uint8_t* ids, hipStream_t s);
// bricks: how many of the bricks the box meets are occupied -> *occupied (device)
hipError_t launch_list_bricks(const ReadBox& b, uint32_t* occupied, hipStream_t s);
// work: list_segments(b) + 1 words (device).  After launch_list_count, work[g] is the first record of segment g and
// work[segments] the number of records; launch_list_scatter then writes the `total` records (nothing at or beyond total).
uint32_t   list_segments(const ReadBox& b);
hipError_t launch_list_count(const ReadBox& b, uint32_t* work, hipStream_t s);
// the scan alone: work[0 .. n) -> its exclusive scan in place, work[n] = the total (vrt_faces.hip scans its own counts with it)
hipError_t launch_list_scan(uint32_t* work, uint32_t n, hipStream_t s);
hipError_t launch_list_scatter(const ReadBox& b, const uint32_t* work, uint32_t total, uint32_t* records, hipStream_t s);
#endif

} // namespace vrt
