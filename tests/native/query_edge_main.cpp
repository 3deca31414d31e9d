// query_edge_main.cpp -- TEST HELPER with its own main: the host build of the ray queries' per-ray code (query_host.cpp) as a
// stand-alone program, so that it can run under AddressSanitizer + UBSan without anything being loaded into another process.
//
//   query_edge_main <rays> <records> <max_steps>...
//
// <rays>: n x 6 packed floats (origin, direction).  The scene is a 40 x 32 x 56 volume from a fixed LCG (qe_fill in query_host.cpp; the test
// fills its own copy through the same function of the un-sanitised library), once as dense fields and once as bricks.  For every budget, first
// on the dense then on the brick scene, <records> receives: material[n] pos[3n] voxel[3n] normal[3n] of the closest hit, (dense
// only) the voxel query_recover_voxel finds [3n], and the any-hit answer [n].  Built and run by tests/test_ray_query_cpu.py.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "query_host.cpp"

int main(int argc, char** argv)
{
    if (argc < 4) { fprintf(stderr, "usage: %s <rays> <records> <max_steps>...\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    const int n = (int)(bytes / 24);
    std::vector<float> rays((size_t)n * 6);
    if (fread(rays.data(), 24, (size_t)n, f) != (size_t)n) { fprintf(stderr, "short read\n"); return 2; }
    fclose(f);
    const int W = 40, H = 32, D = 56;
    std::vector<uint8_t> vol((size_t)W * H * D);
    qe_fill(vol.data(), W, H, D);
    void* dense = th_create(vol.data(), W, H, D);
    void* brick = thb_create(vol.data(), W, H, D);
    FILE* g = fopen(argv[2], "wb");
    if (!g) { perror(argv[2]); return 2; }
    std::vector<uint8_t> out((size_t)n * 41);
    for (int b = 3; b < argc; b++) {
        const uint32_t maxSteps = (uint32_t)strtoul(argv[b], nullptr, 10);
        for (int bricks = 0; bricks < 2; bricks++) {
            const size_t w = qe_records(bricks ? brick : dense, bricks, n, rays.data(), maxSteps, out.data());
            if (fwrite(out.data(), 1, w, g) != w) { fprintf(stderr, "short write\n"); return 2; }
        }
    }
    fclose(g);
    th_destroy(dense); thb_destroy(brick);
    return 0;
}
