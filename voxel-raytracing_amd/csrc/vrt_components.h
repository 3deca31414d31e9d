// vrt_components.h -- which connected components a scene has (vrt_scene_components, vrt_scene_component_labels,
// vrt_scene_filter_components), how they are numbered and measured, and how the device finds them.  Plain integer arithmetic,
// compiled for the device (vrt_components.hip), the host (vrt_api_components.hip) and the tests (tests/native/components_host.cpp,
// components_fuzz.cpp, held against a plain BFS in Python integers, tests/components_reference.py).
//
// DEFINITION.  The BOUNDS are [lo, lo + size) in voxels; lo may be negative, every size in 1..2^30.  They are cut to the volume
// with brush_clip (vrt_brush.h).  Bounds wholly outside the volume have no components and are no error.  A clipped side above
// VRT_COMP_MAX_SIDE = 512 is refused: work in parts.
//   PREDICATE   VRT_COMP_MATCH_SOLID  a voxel passes iff id != 0; two adjacent passing voxels are always joined
//               VRT_COMP_MATCH_SAME   a voxel passes iff id != 0; two adjacent passing voxels are joined iff their ids are equal
//               VRT_COMP_MATCH_EMPTY  a voxel passes iff id == 0; always joined (the cavities and the outer air)
//               (comp_key gives a voxel its KEY, 0 = does not pass; two adjacent voxels are joined iff their keys are equal and
//               not 0.)
//   ADJACENCY   a shared face (VRT_COMP_CONN_FACES = 6) or a face, an edge or a corner (VRT_COMP_CONN_CORNERS = 26), among the
//               voxels OF THE CLIPPED BOUNDS only: what lies outside joins nothing.
//   COMPONENT   a class of the closure of "joined".  The voxel at offset (rx, ry, rz) from the clipped lo has the LINEAR INDEX
//                   L = rx + csize[0] * (ry + csize[1] * rz)                                             (comp_linear; < 2^27)
//               The ROOT of a component is its voxel of lowest L.  Components are NUMBERED 0 .. n-1 in ascending order of their
//               roots' L.  The LABEL of a voxel is its component's number, VRT_COMP_NONE = 0xFFFFFFFF if it does not pass.
//   RECORD      per component (CompRecord, which include/vrt.h mirrors as vrt_component): the root in volume coordinates, the id of
//               the root voxel, the voxel count, the tight box, and `faces`: bit d set iff the component has a voxel on face d of
//               the CLIPPED bounds, d as in vrt_faces.h (0 = -x, 1 = +x, 2 = -y, 3 = +y, 4 = -z, 5 = +z).  A component touches
//               face d iff its tight box does (comp_faces).
//   SELECTION   (the filter) a component is selected iff min_voxels <= count <= max_voxels, (faces & faces_all) == faces_all,
//               (faces & faces_none) == 0 and, under VRT_COMP_FLAG_KEEP_LARGEST, it is not the LARGEST: the component of the
//               highest count, the lowest number among equals (comp_selected).
//
// THE DEVICE'S PASSES.  The label volume is one uint32 per voxel of the clipped bounds at its linear index L, and doubles as the
// PARENT ARRAY P of a union-find: P[L] = VRT_COMP_NONE for a voxel that does not pass, else the linear index of another voxel
// of the same component with P[L] <= L; P[L] == L makes L a root of the forest.
//   1 tile      one wave per 8^3 tile (tiles counted from the clipped lo, as vrt_flood.h's).  Every passing voxel starts with
//               its own L; the wave takes minima over joined neighbours INSIDE the tile until no label changes, so P[L]
//               becomes the lowest L of the voxel's component within the tile (a forest of depth 1).
//   2 seam      every pair of joined voxels that lie in different tiles is united ONCE, by the voxel of the pair from which the
//               other lies in a FORWARD direction (comp_forward: the 3 or 13 directions (dx, dy, dz) with (dz, dy, dx) > 0
//               lexicographically).  unite(a, b) walks both to their roots and, if they differ, links the LARGER root under the
//               smaller with one atomicMin on P[larger]; if that word was no root any more, the walk goes on from the value
//               the atomic returned (which must still be united with the smaller).
//   3 flatten   P[L] becomes the root of L; the roots of every 64-voxel segment of a row (vrt_scene_read.h's segments: ascending
//               segment, then lane, is ascending L) are counted, the counts scanned.
//   4 number    root number k = its segment's first + the roots below it in the segment; the root writes table entry k
//               (CompStat) and P[root] = VRT_COMP_NUMBERED | k.
//   5 measure   one wave per tile: every voxel's P becomes VRT_COMP_NUMBERED | number (read at its root, which this pass never
//               rewrites); per component present in the tile the wave forms count and box by ballots and issues one atomic
//               per statistic (add, min, max): never one per voxel.
//   6 summary   over the table: the largest (max of count << 32 | ~number) and the voxel total.
// The number of launches is constant; no pass is driven by host rounds.
//
// SCHEDULE INDEPENDENCE.  A word of P only ever decreases, and only to the index of a voxel of the same component: pass 1 takes
// minima over joined voxels, pass 2 links a root under a smaller root that a chain of joined voxels connects to it, pass 3
// replaces a parent by an ancestor.  So every set of the final forest lies inside one component.  Conversely unite(a, b)
// returns only after an atomic that found its target a root and linked it -- at that instant a's tree and b's are one -- or
// after finding one root for both; a link that an atomicMin overwrites (P[a]: old -> b, b < old) is not lost, because the
// same call goes on to unite old and b.  After pass 2 each component is therefore ONE tree whatever the order of arrival, and
// since every non-root has a smaller parent, the tree's root is the component's minimum: the root of the definition.  A load
// that returns an out-of-date word returns a value the word once held, which is an ancestor-to-be in the same component and
// smaller than the index: the walk still ends at a candidate root, and the atomic (which sees the word as it is) decides.
// Numbers follow from the roots alone; counts and boxes are integer add / min / max, the face bits follow from the boxes, and
// the largest is a max over distinct keys: all independent of the order.  No wave waits for another: no locks, no flags, no
// barriers between workgroups.
//
// THE LOOP BOUND.  Every step of a walk (comp_find) and every turn of unite's loop moves to a strictly smaller index, so a
// walk from L ends within L steps and a unite of (a, b) within a + b turns.  Builds with VRT_COMP_DEBUG count the steps and
// stop a walk that exceeds its bound (the result is then wrong and the tests see it); product builds carry no check.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <vector>

#if defined(__HIPCC__)
#define VRT_COMP_HD __host__ __device__ inline
#else
#define VRT_COMP_HD inline
#endif

// (include/vrt.h has the same values for the C-ABI; vrt_api_components.hip asserts that they agree)
#define VRT_COMP_MATCH_SOLID 0
#define VRT_COMP_MATCH_SAME 1
#define VRT_COMP_MATCH_EMPTY 2
#define VRT_COMP_CONN_FACES 6
#define VRT_COMP_CONN_CORNERS 26
#define VRT_COMP_FLAG_KEEP_LARGEST 1u     // the filter's flags
#define VRT_COMP_FLAG_MEASURE 2u

#define VRT_COMP_MAX_SIDE 512u            // voxels, of the clipped bounds
#define VRT_COMP_MAX_SIZE (1u << 30)      // of the bounds as given
#define VRT_COMP_TILE 8u
#define VRT_COMP_NONE 0xFFFFFFFFu         // the label of a voxel that does not pass
#define VRT_COMP_NUMBERED 0x80000000u     // device, passes 4 to 6: the word holds a component number, not a parent (numbers are < 2^27)

namespace vrt {

// One component, as vrt_scene_components lists it (include/vrt.h: vrt_component; 56 bytes)
struct CompRecord {
    int32_t  root[3];            // volume coordinates
    uint32_t id;                 // of the root voxel
    uint64_t voxels;
    int32_t  lo[3];              // the tight box, volume coordinates
    uint32_t size[3];
    uint32_t faces;              // bit d: touches face d of the clipped bounds
    uint32_t reserved;           // 0
};

// The device's table entry: offsets from the clipped lo, max inclusive.  Pass 4 writes root, id and the neutral elements
// (count 0, mn 0xFFFFFFFF, mx 0), pass 5 accumulates, the filter's selection sets `selected`.
struct CompStat {
    uint32_t root;               // linear index
    uint32_t id;
    uint32_t count;              // <= 2^27
    uint32_t mn[3], mx[3];
    uint32_t selected;
};

VRT_COMP_HD bool comp_match_ok(int32_t match) { return match == VRT_COMP_MATCH_SOLID || match == VRT_COMP_MATCH_SAME || match == VRT_COMP_MATCH_EMPTY; }
VRT_COMP_HD bool comp_conn_ok(int32_t c) { return c == VRT_COMP_CONN_FACES || c == VRT_COMP_CONN_CORNERS; }

// vrt_components: no flag is defined yet
VRT_COMP_HD bool comp_args_ok(int32_t match, int32_t connectivity, uint32_t flags, const uint32_t size[3])
{
    if (!comp_match_ok(match) || !comp_conn_ok(connectivity) || flags != 0u) return false;
    for (int a = 0; a < 3; a++)
        if (size[a] < 1u || size[a] > VRT_COMP_MAX_SIZE) return false;
    return true;
}

VRT_COMP_HD bool comp_filter_ok(uint64_t min_voxels, uint64_t max_voxels, uint32_t faces_all, uint32_t faces_none, uint32_t flags)
{
    return min_voxels <= max_voxels && ((faces_all | faces_none) & ~63u) == 0u && (flags & ~(VRT_COMP_FLAG_KEEP_LARGEST | VRT_COMP_FLAG_MEASURE)) == 0u;
}

VRT_COMP_HD bool comp_sides_ok(const uint32_t csize[3])
{
    return csize[0] <= VRT_COMP_MAX_SIDE && csize[1] <= VRT_COMP_MAX_SIDE && csize[2] <= VRT_COMP_MAX_SIDE;
}

// 0: the voxel does not pass; two adjacent voxels are joined iff their keys are equal and not 0
VRT_COMP_HD uint32_t comp_key(int32_t match, uint32_t id)
{
    if (match == VRT_COMP_MATCH_EMPTY) return id == 0u ? 1u : 0u;
    if (match == VRT_COMP_MATCH_SAME) return id;
    return id != 0u ? 1u : 0u;
}

VRT_COMP_HD uint32_t comp_linear(uint32_t rx, uint32_t ry, uint32_t rz, const uint32_t csize[3]) { return rx + csize[0] * (ry + csize[1] * rz); }

VRT_COMP_HD void comp_tiles(const uint32_t csize[3], uint32_t nt[3])
{
    for (int a = 0; a < 3; a++) nt[a] = (csize[a] + VRT_COMP_TILE - 1u) / VRT_COMP_TILE;
}

// the forward directions: k in 0 .. comp_forward_count, (dx, dy, dz) with (dz, dy, dx) > 0 lexicographically
VRT_COMP_HD uint32_t comp_forward_count(int32_t connectivity) { return connectivity == VRT_COMP_CONN_FACES ? 3u : 13u; }
VRT_COMP_HD void comp_forward(int32_t connectivity, uint32_t k, int d[3])
{
    if (connectivity == VRT_COMP_CONN_FACES) { d[0] = k == 0u; d[1] = k == 1u; d[2] = k == 2u; return; }
    const uint32_t c = k + 14u;                                   // the cells of the 3^3 block behind its centre (13), x fastest
    d[0] = (int)(c % 3u) - 1; d[1] = (int)((c / 3u) % 3u) - 1; d[2] = (int)(c / 9u) - 1;
}

// the faces of the clipped bounds that the box [mn, mx] (offsets from the clipped lo, max inclusive) touches
VRT_COMP_HD uint32_t comp_faces(const uint32_t mn[3], const uint32_t mx[3], const uint32_t csize[3])
{
    uint32_t f = 0u;
    for (int a = 0; a < 3; a++) {
        if (mn[a] == 0u) f |= 1u << (2 * a);
        if (mx[a] == csize[a] - 1u) f |= 2u << (2 * a);
    }
    return f;
}

VRT_COMP_HD bool comp_selected(uint64_t count, uint32_t faces, bool largest, uint64_t min_voxels, uint64_t max_voxels, uint32_t faces_all, uint32_t faces_none, uint32_t flags)
{
    if (count < min_voxels || count > max_voxels) return false;
    if ((faces & faces_all) != faces_all || (faces & faces_none) != 0u) return false;
    return !((flags & VRT_COMP_FLAG_KEEP_LARGEST) != 0u && largest);
}

// the key the largest component maximises: the count, then the LOWER number
VRT_COMP_HD uint64_t comp_largest_key(uint32_t count, uint32_t number) { return ((uint64_t)count << 32) | (uint64_t)(0xFFFFFFFFu - number); }
VRT_COMP_HD uint32_t comp_largest_number(uint64_t key) { return 0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFull); }

// (Hidden: an out-of-line copy stays out of libvrt_hip.so's dynamic symbols.)
__attribute__((visibility("hidden"))) VRT_COMP_HD CompRecord comp_record_of(const CompStat& t, const int32_t clo[3], const uint32_t csize[3])
{
    CompRecord r{};
    const uint32_t o[3] = {t.root % csize[0], (t.root / csize[0]) % csize[1], t.root / (csize[0] * csize[1])};
    for (int a = 0; a < 3; a++) {
        r.root[a] = clo[a] + (int32_t)o[a];
        r.lo[a] = clo[a] + (int32_t)t.mn[a];
        r.size[a] = t.mx[a] - t.mn[a] + 1u;
    }
    r.id = t.id; r.voxels = t.count; r.faces = comp_faces(t.mn, t.mx, csize);
    return r;
}

// ---- the whole definition on the host, sequentially: the twin the native tests run ------------------------------------------------

// the root of x in the parent array p; every step goes to a smaller index
inline uint32_t comp_find_host(const std::vector<uint32_t>& p, uint32_t x)
{
    while (p[x] != x) x = p[x];
    return x;
}

// ids: the clipped bounds' voxels at their linear indices.  -> labels (one per voxel) and the table in component order;
// *largest: the number of the largest component (0 when there is none), *voxels: the passing voxels
inline void comp_label_host(const uint8_t* ids, const uint32_t csize[3], int32_t match, int32_t connectivity, std::vector<uint32_t>& labels,
                            std::vector<CompStat>& table, uint64_t* largest, uint64_t* voxels)
{
    const size_t n = (size_t)csize[0] * csize[1] * csize[2];
    std::vector<uint32_t> p(n);
    for (size_t i = 0; i < n; i++) p[i] = comp_key(match, ids[i]) != 0u ? (uint32_t)i : VRT_COMP_NONE;
    const uint32_t nd = comp_forward_count(connectivity);
    for (uint32_t rz = 0; rz < csize[2]; rz++) for (uint32_t ry = 0; ry < csize[1]; ry++) for (uint32_t rx = 0; rx < csize[0]; rx++) {
        const uint32_t L = comp_linear(rx, ry, rz, csize), key = comp_key(match, ids[L]);
        if (key == 0u) continue;
        for (uint32_t k = 0; k < nd; k++) {
            int d[3];
            comp_forward(connectivity, k, d);
            const int64_t nx = (int64_t)rx + d[0], ny = (int64_t)ry + d[1], nz = (int64_t)rz + d[2];
            if (nx < 0 || nx >= (int64_t)csize[0] || ny < 0 || ny >= (int64_t)csize[1] || nz >= (int64_t)csize[2]) continue;
            const uint32_t M = comp_linear((uint32_t)nx, (uint32_t)ny, (uint32_t)nz, csize);
            if (comp_key(match, ids[M]) != key) continue;
            uint32_t a = comp_find_host(p, L), b = comp_find_host(p, M);
            if (a == b) continue;
            if (a < b) { const uint32_t t = a; a = b; b = t; }
            p[a] = b;                                              // the larger root under the smaller
        }
    }
    labels.assign(n, VRT_COMP_NONE);
    table.clear();
    for (size_t i = 0; i < n; i++) {                              // ascending L: a root is numbered before any other voxel of its component is met
        if (p[i] == VRT_COMP_NONE) continue;
        const uint32_t r = comp_find_host(p, (uint32_t)i);
        if (r == (uint32_t)i) {
            CompStat t{};
            t.root = r; t.id = ids[i];
            for (int a = 0; a < 3; a++) { t.mn[a] = 0xFFFFFFFFu; t.mx[a] = 0u; }
            labels[i] = (uint32_t)table.size();
            table.push_back(t);
        } else labels[i] = labels[r];
        CompStat& t = table[labels[i]];
        const uint32_t o[3] = {(uint32_t)(i % csize[0]), (uint32_t)((i / csize[0]) % csize[1]), (uint32_t)(i / ((size_t)csize[0] * csize[1]))};
        t.count++;
        for (int a = 0; a < 3; a++) { if (o[a] < t.mn[a]) t.mn[a] = o[a]; if (o[a] > t.mx[a]) t.mx[a] = o[a]; }
    }
    uint64_t best = 0, total = 0;
    for (size_t k = 0; k < table.size(); k++) {
        const uint64_t key = comp_largest_key(table[k].count, (uint32_t)k);
        if (key > best) best = key;
        total += table[k].count;
    }
    *largest = table.empty() ? 0ull : (uint64_t)comp_largest_number(best);
    *voxels = total;
}

} // namespace vrt
