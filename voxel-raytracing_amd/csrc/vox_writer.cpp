// vox_writer.cpp -- MagicaVoxel .vox serialisation of a scene: the inverse of vox_reader.cpp (and of the reference's load,
// source/voxels/resource/voxel_scene.cpp:9-31,53-117 over ogt_vox.h:1179-1991).  Written from the published .vox format.
//
// The file, in this order: "VOX " 200, MAIN; one SIZE / XYZI pair per tile; the scene graph (root nTRN 0 -> nGRP 1, and per
// tile k an nTRN 2 + 2k -> nSHP 3 + 2k); RGBA; one MATL per metallic material.
//   Tiles   the scene (W, H, D) cut into boxes of at most 256 per axis, the last of an axis taking the remainder, x fastest,
//           then y, then z (vrt_scene_read.h).  EVERY tile is written: the loaders take the scene's extent from the corners of
//           the model instances, so a tile that is left out at the rim would shrink the scene.  Both loaders drop a model whose
//           XYZI chunk has no record (ogt_vox.h:1263,1299-1301; vox_reader.cpp does the same), so an empty tile carries ONE
//           record, voxel (0, 0, 0) with colour index 0 -- which is the empty voxel: the model is kept, its corners count, and
//           it stores nothing.
//   Axes    file x = scene x, file y = scene z, file z = scene y (the load's swap, voxel_scene.cpp:72-74,99): SIZE is
//           (tw, td, th) and a record's bytes are (x, z, y, id).
//   _t      a tile's translation is its corner plus floor(size / 2) per FILE axis (calc_vox_pivot), rotation identity:
//           floor(p + 0.5 - pivot + t) is then p + corner for every voxel, and the two corners of the tiles span exactly
//           [0, W) x [0, D) x [0, H) in file axes -- for odd sizes and for size 1 (pivot 0) alike.
//   RGBA    entry i colours id i + 1; entry 255 is id 0's colour (the loaders rotate the palette and zero id 0's alpha).  A
//           channel's byte is vox_colour_byte of its float.
//   MATL    for metallic != 0: _type _metal, _metal printed with %.9g, which atof + the cast to float read back exactly.
//
// CONTRACT: a scene whose palette came from bytes -- every loaded .vox -- reads back exactly: voxels, dims, every palette
// float, every metallic value.  ANY OTHER PALETTE IS QUANTISED to the nearest colour a byte can express (id 0's alpha reads
// back as 0 whatever it was), and the file cannot exceed the 2^32 - 1 bytes a MAIN chunk's child size (and the loaders' 32-bit
// buffer size) can state.
#include "vox_writer.h"

#include <cmath>
#include <cstdio>
#include <cstring>

#include "vrt_scene_read.h"

namespace vrt {
namespace {

void put32(std::vector<uint8_t>& o, uint32_t v) { uint8_t b[4]; memcpy(b, &v, 4); o.insert(o.end(), b, b + 4); }
void put_str(std::vector<uint8_t>& o, const char* s) { const size_t n = strlen(s); put32(o, (uint32_t)n); o.insert(o.end(), s, s + n); }

// a chunk's header; returns where its content begins (end_chunk patches the content size)
size_t begin_chunk(std::vector<uint8_t>& o, const char id[5])
{
    o.insert(o.end(), id, id + 4);
    put32(o, 0); put32(o, 0);
    return o.size();
}
void end_chunk(std::vector<uint8_t>& o, size_t content)
{
    const uint32_t n = (uint32_t)(o.size() - content);
    memcpy(&o[content - 8], &n, 4);
}

// the loader's float of every byte (vox_reader.cpp; voxel_scene.cpp:114-115)
const float* colour_table()
{
    static float table[256];
    static bool made = false;
    if (!made) {
        for (int c = 0; c < 256; c++) table[c] = powf((float)c / 255.0f, 2.2f);
        made = true;
    }
    return table;
}

} // namespace

uint8_t vox_colour_byte(float v)
{
    const float* t = colour_table();
    if (v != v) return 0;
    int best = 0;
    double best_d = fabs((double)t[0] - (double)v);
    for (int c = 0; c < 256; c++) {
        if (memcmp(&t[c], &v, 4) == 0) return (uint8_t)c;
        const double d = fabs((double)t[c] - (double)v);
        if (d < best_d) { best = c; best_d = d; }              // strictly nearer only: a tie keeps the lower byte
    }
    return (uint8_t)best;
}

void VoxWriter::begin(const uint32_t dims[3])
{
    out.clear();
    next_ = 0; too_big_ = false;
    for (int a = 0; a < 3; a++) { dims_[a] = dims[a]; nt_[a] = save_tiles(dims[a]); }
    const char magic[5] = "VOX ";
    out.insert(out.end(), magic, magic + 4);
    put32(out, 200);
    begin_chunk(out, "MAIN");                                   // content 0; finish() states the children's size
}

void VoxWriter::tile_box(uint32_t t, int32_t lo[3], uint32_t size[3]) const
{
    const uint32_t k[3] = {t % nt_[0], (t / nt_[0]) % nt_[1], t / (nt_[0] * nt_[1])};
    for (int a = 0; a < 3; a++) { uint32_t l; save_tile_span(dims_[a], k[a], &l, &size[a]); lo[a] = (int32_t)l; }
}

bool VoxWriter::room(size_t more)
{
    if (too_big_ || more > 0xFFFFFFFFull || out.size() + more > 0xFFFFFFFFull) too_big_ = true;
    return !too_big_;
}

void VoxWriter::tile(const uint32_t* records, size_t n)
{
    int32_t lo[3]; uint32_t size[3];
    tile_box(next_++, lo, size);
    const size_t nrec = n ? n : 1;                              // an empty tile: one record with colour index 0 (see the top)
    if (nrec > 0x3FFFFFFFull || !room(24 + 16 + nrec * 4)) { too_big_ = true; return; }
    size_t c = begin_chunk(out, "SIZE");
    put32(out, size[0]); put32(out, size[2]); put32(out, size[1]);
    end_chunk(out, c);
    c = begin_chunk(out, "XYZI");
    put32(out, (uint32_t)nrec);
    const size_t at = out.size();
    out.resize(at + nrec * 4, 0);
    for (size_t i = 0; i < n; i++) {
        const uint32_t r = records[i];
        uint8_t* b = &out[at + i * 4];
        b[0] = (uint8_t)r; b[1] = (uint8_t)(r >> 16); b[2] = (uint8_t)(r >> 8); b[3] = (uint8_t)(r >> 24);
    }
    end_chunk(out, c);
}

int VoxWriter::finish(const vrt_material palette[256], std::string& err)
{
    const uint32_t nt = tiles();
    std::vector<uint8_t> tail;
    // root transform -> the one group -> a transform and a shape per tile
    size_t c = begin_chunk(tail, "nTRN");
    put32(tail, 0); put32(tail, 0); put32(tail, 1); put32(tail, 0xFFFFFFFFu); put32(tail, 0xFFFFFFFFu); put32(tail, 1); put32(tail, 0);
    end_chunk(tail, c);
    c = begin_chunk(tail, "nGRP");
    put32(tail, 1); put32(tail, 0); put32(tail, nt);
    for (uint32_t k = 0; k < nt; k++) put32(tail, 2 + 2 * k);
    end_chunk(tail, c);
    for (uint32_t k = 0; k < nt; k++) {
        int32_t lo[3]; uint32_t size[3];
        tile_box(k, lo, size);
        char t[64];
        snprintf(t, sizeof t, "%d %d %d", lo[0] + (int)(size[0] / 2), lo[2] + (int)(size[2] / 2), lo[1] + (int)(size[1] / 2));
        c = begin_chunk(tail, "nTRN");
        put32(tail, 2 + 2 * k); put32(tail, 0); put32(tail, 3 + 2 * k); put32(tail, 0xFFFFFFFFu); put32(tail, 0); put32(tail, 1);
        put32(tail, 1); put_str(tail, "_t"); put_str(tail, t);
        end_chunk(tail, c);
        c = begin_chunk(tail, "nSHP");
        put32(tail, 3 + 2 * k); put32(tail, 0); put32(tail, 1); put32(tail, k); put32(tail, 0);
        end_chunk(tail, c);
    }
    c = begin_chunk(tail, "RGBA");
    for (int i = 0; i < 256; i++) {
        const vrt_material& m = palette[(i + 1) & 255];
        for (int k = 0; k < 4; k++) tail.push_back(vox_colour_byte(m.diffuse[k]));
    }
    end_chunk(tail, c);
    for (int id = 0; id < 256; id++) {
        if (!(palette[id].metallic != 0.0f)) continue;
        char v[64];
        snprintf(v, sizeof v, "%.9g", (double)palette[id].metallic);
        c = begin_chunk(tail, "MATL");
        put32(tail, id ? (uint32_t)id : 256u);                  // the format counts materials 1 .. 256; 256 is id 0
        put32(tail, 2); put_str(tail, "_type"); put_str(tail, "_metal"); put_str(tail, "_metal"); put_str(tail, v);
        end_chunk(tail, c);
    }
    if (!too_big_ && next_ != nt) { err = "vox writer: internal error (tiles)"; return VRT_ERR_INVALID; }
    if (!room(tail.size())) {
        out.clear();
        err = "the scene has more non-empty voxels than a .vox file can hold (a MAIN chunk states its children's size in 32 bits)";
        return VRT_ERR_UNSUPPORTED;
    }
    out.insert(out.end(), tail.begin(), tail.end());
    const uint32_t children = (uint32_t)(out.size() - 20);
    memcpy(&out[16], &children, 4);
    return VRT_OK;
}

int vox_encode(const uint8_t* voxels, const uint32_t dims[3], const vrt_material palette[256], std::vector<uint8_t>& out, std::string& err)
{
    VoxWriter w;
    w.begin(dims);
    std::vector<uint32_t> rec;
    for (uint32_t t = 0; t < w.tiles(); t++) {
        int32_t lo[3]; uint32_t size[3];
        w.tile_box(t, lo, size);
        rec.clear();
        for (uint32_t bz = 0; bz < size[2]; bz++) for (uint32_t by = 0; by < size[1]; by++) {
            const uint8_t* row = voxels + (size_t)lo[0] + ((size_t)(lo[1] + by) + (size_t)(lo[2] + bz) * dims[1]) * dims[0];
            for (uint32_t bx = 0; bx < size[0]; bx++)
                if (row[bx]) rec.push_back(list_record(bx, by, bz, row[bx]));
        }
        w.tile(rec.data(), rec.size());
    }
    const int rc = w.finish(palette, err);
    if (rc == VRT_OK) out.swap(w.out);
    return rc;
}

} // namespace vrt
