// vrt_faces.h -- surface extraction (vrt_scene_list_faces, vrt_faces_mesh_host, the OBJ writer): which faces of a box's voxels are
// exposed, how they merge into runs, the record a run becomes, the order of the records and the quad of a record.  Plain integer
// arithmetic, compiled for the device (vrt_faces.hip), the host (vrt_api_faces.hip) and the tests (tests/native/faces_host.cpp,
// which is held against a numpy restatement).  The box, its checks and the word of a voxel are vrt_scene_read.h's.
//
// DIRECTIONS d: 0 = -x, 1 = +x, 2 = -y, 3 = +y, 4 = -z, 5 = +z; axis(d) = d / 2.  Face d of a voxel of the box with id != 0 is
// EXPOSED iff the voxel across it is empty.  A neighbour outside the volume is empty; a neighbour outside the box but inside the
// volume is read from the scene, so a scene extracted in parts gives the faces of the scene extracted whole -- unless
// VRT_FACES_CLOSED is set, under which every voxel outside the box is empty (face_neighbour_reads).
//
// The RUN AXIS u(d) is y for d < 2 and x otherwise (face_run_axis); the ORDER KEY of a voxel for direction d has the run axis
// fastest: read_box_index for d >= 2, by + (bx + bz * size[0]) * size[1] for d < 2 (face_order_key).  Without VRT_FACES_RUNS every
// exposed face is a record of length 1.  With it, an exposed face CONTINUES the exposed face of the same d one step below it along
// u(d) iff both voxels have the same id and its own box-relative u is no multiple of VRT_LIST_SEGMENT = 64; a run is a maximal
// chain (length 1 .. 64) and becomes one record.  The break at 64 is part of the definition: it lets one wave own a run.
//
// A RECORD is one uint64_t: list_record(bx, by, bz, id) of the run's lowest voxel in bits 0 .. 31, length - 1 in bits 32 .. 37,
// d in bits 40 .. 42, every other bit 0 (face_record).  The records come in ascending d, within a d in ascending order key of
// their first voxel.  The order is part of the contract: the output is a function of the scene's content, the box and the flags.
// The kernels keep it without sorting, as vrt_scene_list_box does: for direction d the box is cut into SEGMENTS of 64 voxels
// along u(d) (face_segments of them, numbered in order-key order: face_segment_voxel), one wave takes a segment, and an exclusive
// scan over the (direction, segment) counts -- direction-major -- gives every segment's first record.  A direction has at most
// 256^3 / 2 = 2^23 exposed faces and a call at most 6 * 2^23 < 2^26 records, so 32-bit scan words suffice.
//
// The QUAD of a record lies in the plane axis(d) = coordinate (+ 1 for odd d), is `length` long along u(d) and 1 along the third
// axis w(d) (face_third_axis).  Its four corners start at the corner with the lowest coordinates and run counter-clockwise seen
// from the empty side, so (corner 1 - corner 0) x (corner 3 - corner 0) points along d.  face_corner(d, k) has the table: bit 0 =
// the corner lies at the far end along u, bit 1 = along w.
#pragma once

#include "vrt_scene_read.h"

#define VRT_FACES_FLAG_RUNS   1u     // (include/vrt.h: VRT_FACES_RUNS, VRT_FACES_CLOSED)
#define VRT_FACES_FLAG_CLOSED 2u
#define VRT_FACES_DIRECTIONS  6u

namespace vrt {

VRT_READ_HD uint32_t face_axis(uint32_t d) { return d >> 1; }
VRT_READ_HD uint32_t face_run_axis(uint32_t d) { return d < 2u ? 1u : 0u; }
VRT_READ_HD uint32_t face_third_axis(uint32_t d) { return d < 4u ? 2u : 1u; }

VRT_READ_HD size_t face_order_key(uint32_t d, uint32_t bx, uint32_t by, uint32_t bz, const uint32_t size[3])
{
    if (d >= 2u) return read_box_index(bx, by, bz, size);
    return (size_t)by + ((size_t)bx + (size_t)bz * (size_t)size[0]) * (size_t)size[1];
}

// segments of direction d, and the voxel of lane `lane` of segment g (false: beyond the end of its row)
VRT_READ_HD uint32_t face_segments(uint32_t d, const uint32_t size[3])
{
    return d < 2u ? list_segments_per_row(size[1]) * size[0] * size[2] : list_segments_per_row(size[0]) * size[1] * size[2];
}

VRT_READ_HD bool face_segment_voxel(uint32_t d, uint32_t g, uint32_t lane, const uint32_t size[3], uint32_t* bx, uint32_t* by, uint32_t* bz)
{
    if (d < 2u) {                                                   // rows along y: x next, then z
        const uint32_t spr = list_segments_per_row(size[1]), row = g / spr;
        *by = (g - row * spr) * VRT_LIST_SEGMENT + lane;
        *bz = row / size[0];
        *bx = row - *bz * size[0];
        return *by < size[1];
    }
    const uint32_t spr = list_segments_per_row(size[0]), row = g / spr;
    *bx = (g - row * spr) * VRT_LIST_SEGMENT + lane;
    *bz = row / size[1];
    *by = row - *bz * size[1];
    return *bx < size[0];
}

// The voxel across face d of box voxel b (box-relative, may leave the box by one): 0 = it is empty without a look at the scene
// (outside the volume, or outside the box under CLOSED), 1 = read volume voxel p
VRT_READ_HD int face_neighbour_reads(uint32_t d, const int32_t b[3], const int32_t lo[3], const uint32_t size[3], const int32_t dim[3],
                                     uint32_t flags, int32_t p[3])
{
    const uint32_t a = face_axis(d);
    int32_t n[3] = {b[0], b[1], b[2]};
    n[a] += (d & 1u) ? 1 : -1;
    for (int k = 0; k < 3; k++) p[k] = lo[k] + n[k];
    if (p[a] < 0 || p[a] >= dim[a]) return 0;
    if ((flags & VRT_FACES_FLAG_CLOSED) && (n[a] < 0 || n[a] >= (int32_t)size[a])) return 0;
    return 1;
}

VRT_READ_HD uint64_t face_record(uint32_t bx, uint32_t by, uint32_t bz, uint32_t id, uint32_t length, uint32_t d)
{
    return (uint64_t)list_record(bx, by, bz, id) | ((uint64_t)(length - 1u) << 32) | ((uint64_t)d << 40);
}

VRT_READ_HD uint32_t face_record_d(uint64_t r) { return (uint32_t)(r >> 40) & 7u; }
VRT_READ_HD uint32_t face_record_length(uint64_t r) { return ((uint32_t)(r >> 32) & 63u) + 1u; }
VRT_READ_HD uint32_t face_record_id(uint64_t r) { return (uint32_t)(r >> 24) & 255u; }
// a word a call can have written: no stray bit, a direction, a non-empty id
VRT_READ_HD bool face_record_valid(uint64_t r)
{
    return (r & ~0x0000073FFFFFFFFFull) == 0u && face_record_d(r) < VRT_FACES_DIRECTIONS && face_record_id(r) != 0u;
}

// corner k (0 .. 3) of the quad of direction d: bit 0 = at the far end along u(d), bit 1 = at the far end along w(d).  With
// u x w = +axis for d < 2 (y x z) and d >= 4 (x x y) and -axis for d = 2, 3 (x x z), the corners run u first for d = 1, 2, 5.
VRT_READ_HD uint32_t face_corner(uint32_t d, uint32_t k)
{
    const bool u_first = d == 1u || d == 2u || d == 5u;
    const uint32_t table = u_first ? 0x2310u : 0x1320u;             // corner k in nibble k: (0,0) (u,0) (u,w) (0,w) or (0,0) (0,w) (u,w) (u,0)
    return (table >> (4u * k)) & 3u;
}

// corner k of record r's quad, in voxels relative to the box's lo
VRT_READ_HD void face_quad_corner(uint64_t r, uint32_t k, uint32_t c[3])
{
    const uint32_t d = face_record_d(r), bits = face_corner(d, k);
    c[0] = (uint32_t)r & 255u; c[1] = (uint32_t)(r >> 8) & 255u; c[2] = (uint32_t)(r >> 16) & 255u;
    c[face_axis(d)] += d & 1u;
    if (bits & 1u) c[face_run_axis(d)] += face_record_length(r);
    if (bits & 2u) c[face_third_axis(d)] += 1u;
}

} // namespace vrt
