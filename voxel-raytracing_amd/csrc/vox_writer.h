// vox_writer.h -- host-side .vox serialiser (see vox_writer.cpp).
#pragma once

#include <stdint.h>
#include <string>
#include <vector>

#include "../../include/vrt.h"

namespace vrt {

// A scene of dims (W, H, D) as a MagicaVoxel file, tile by tile: begin(), one tile() per tile in the order of
// vrt_scene_read.h (x fastest, then y, then z) with the tile's records in vrt_scene_list_box order, then finish().
class VoxWriter {
public:
    void begin(const uint32_t dims[3]);
    uint32_t tiles() const { return nt_[0] * nt_[1] * nt_[2]; }
    // the box of tile t in scene coordinates
    void tile_box(uint32_t t, int32_t lo[3], uint32_t size[3]) const;
    // the next tile's model: n records (x | y << 8 | z << 16 | id << 24 in scene axes, relative to the tile's corner)
    void tile(const uint32_t* records, size_t n);
    // scene graph, palette, materials; VRT_OK, or VRT_ERR_UNSUPPORTED when the file passes what a MAIN chunk can hold
    int finish(const vrt_material palette[256], std::string& err);
    bool too_big() const { return too_big_; }
    std::vector<uint8_t> out;

private:
    bool room(size_t more);
    uint32_t dims_[3] = {0, 0, 0}, nt_[3] = {0, 0, 0}, next_ = 0;
    bool too_big_ = false;
};

// The byte c whose pow(c / 255, 2.2) -- the loader's float -- is v bit for bit; else the byte whose float is nearest to v,
// ties to the lower byte (NaN: 0)
uint8_t vox_colour_byte(float v);

// The whole file from a dense volume (x + y*W + z*W*H) -- what VoxWriter makes of its tiles
int vox_encode(const uint8_t* voxels, const uint32_t dims[3], const vrt_material palette[256], std::vector<uint8_t>& out, std::string& err);

} // namespace vrt
