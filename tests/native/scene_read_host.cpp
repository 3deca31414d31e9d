// Host build of csrc/vrt_scene_read.h for tests/test_vox_writer_cpu.py: the records of a box of a dense volume, made by walking
// the header's SEGMENTS the way the kernels do (ascending segment, ascending lane, list_record), to be held against numpy's
// np.nonzero in index order; and the header's checks of a box and its tiles.
#include <cstdint>

#include "../../voxel-raytracing_amd/csrc/vrt_scene_read.h"

using namespace vrt;

extern "C" {

// vol: dims[0] * dims[1] * dims[2] ids, x fastest.  Returns the number of records (written while they fit `capacity`), or -1 - the
// check's code for a box the header refuses
long long scene_read_list(const uint8_t* vol, const int32_t dims[3], const int32_t lo[3], const uint32_t size[3], uint32_t* records,
                          unsigned long long capacity)
{
    size_t n = 0;
    const ReadBoxCheck k = read_box_check(dims, lo, size, VRT_LIST_MAX_SIDE, &n);
    if (k != READ_BOX_OK) return -1 - (long long)k;
    const uint32_t spr = list_segments_per_row(size[0]), nseg = spr * size[1] * size[2];
    unsigned long long out = 0;
    uint32_t expect = 0;
    for (uint32_t bz = 0; bz < size[2]; bz++) for (uint32_t by = 0; by < size[1]; by++) for (uint32_t s = 0; s < spr; s++) {
        if (list_segment(s * VRT_LIST_SEGMENT, by, bz, size) != expect++) return -100;      // segments ascend with the box index
        for (uint32_t lane = 0; lane < VRT_LIST_SEGMENT; lane++) {
            const uint32_t bx = s * VRT_LIST_SEGMENT + lane;
            if (bx >= size[0]) break;
            const uint8_t id = vol[(size_t)(lo[0] + (int)bx) + ((size_t)(lo[1] + (int)by) + (size_t)(lo[2] + (int)bz) * dims[1]) * dims[0]];
            if (!id) continue;
            if (out < capacity) records[out] = list_record(bx, by, bz, id);
            out++;
        }
    }
    return expect == nseg ? (long long)out : -100;
}

// the check alone (max_side 0: vrt_scene_read_box's, 256: vrt_scene_list_box's); *count as the header leaves it
int scene_read_check(const int32_t dims[3], const int32_t lo[3], const uint32_t size[3], uint32_t max_side, unsigned long long* count)
{
    size_t n = 0;
    const int k = (int)read_box_check(dims, lo, size, max_side, &n);
    *count = n;
    return k;
}

unsigned long long scene_read_index(uint32_t bx, uint32_t by, uint32_t bz, const uint32_t size[3]) { return read_box_index(bx, by, bz, size); }

// tiles of an axis: returns their number, and tile t's span
uint32_t scene_read_tiles(uint32_t dim, uint32_t t, uint32_t* lo, uint32_t* size)
{
    if (t < save_tiles(dim)) save_tile_span(dim, t, lo, size);
    return save_tiles(dim);
}

}
