// brush_limits_main.cpp -- TEST HELPER with its own main, built and run by tests/test_gpu_brush_limits.py: the C++ mirror's
// VoxelScene::brush and VoxelScene::stamp (voxel-raytracing_amd/host/voxels.hpp) on two volumes read from files.
//   brush_limits_main <dst.u8> W H D <src.u8> w h d <out.vox>
// One brush on the destination, the whole source stamped onto it, a box of the source stamped turned with skipEmpty; prints one
// line "result changed lo[3] size[3]" per call and saves the destination as out.vox.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <iterator>

#include "../../voxel-raytracing_amd/host/voxels.hpp"

using namespace vrt_host;

static std::vector<uint8_t> load(const char* path, size_t n)
{
    std::ifstream f(path, std::ios::binary);
    std::vector<uint8_t> v((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    if (v.size() != n) throw std::runtime_error(std::string("unexpected size of ") + path);
    return v;
}

static void print(const vrt_brush_result& r)
{
    std::printf("result %llu %d %d %d %u %u %u\n", (unsigned long long)r.changed, r.lo[0], r.lo[1], r.lo[2], r.size[0], r.size[1], r.size[2]);
}

int main(int argc, char** argv)
{
    if (argc != 10) { std::fprintf(stderr, "usage: brush_limits_main <dst.u8> W H D <src.u8> w h d <out.vox>\n"); return 2; }
    try {
        const uint32_t W = (uint32_t)std::atoi(argv[2]), H = (uint32_t)std::atoi(argv[3]), D = (uint32_t)std::atoi(argv[4]);
        const uint32_t w = (uint32_t)std::atoi(argv[6]), h = (uint32_t)std::atoi(argv[7]), d = (uint32_t)std::atoi(argv[8]);
        const std::vector<uint8_t> dstv = load(argv[1], (size_t)W * H * D), srcv = load(argv[5], (size_t)w * h * d);
        std::vector<vrt_material> pal(256);
        for (int i = 0; i < 256; i++) {
            pal[i] = vrt_material{};
            pal[i].diffuse[0] = (float)i / 255.0f; pal[i].diffuse[1] = 0.5f; pal[i].diffuse[2] = 1.0f - (float)i / 255.0f; pal[i].diffuse[3] = 1.0f;
        }
        auto engine = std::make_shared<Engine>(0);
        VoxelScene dst(engine, dstv.data(), W, H, D, pal.data()), src(engine, srcv.data(), w, h, d, pal.data());
        // an ellipsoid with one semi-axis at the limit, centred on voxel (20, 11.5, 16)
        print(dst.ellipsoid({20.5, 12.0, 16.5}, {6.5, 4.5, 512.0}, 77, VRT_BRUSH_ADD));
        print(dst.stamp({-2, 3, 20}, src, {0, 0, 0}, {w, h, d}));
        print(dst.stamp({30, -4, 1}, src, {1, 2, 3}, {15, 6, 7}, 3u | 5u << 3, true));
        dst.save(argv[9]);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
