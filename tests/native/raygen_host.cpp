// raygen_host.cpp -- TEST HELPER: the ray generators of vrt_camera_rays (csrc/vrt_raygen.h) compiled for the host, so that the
// definition the kernel runs can be compared with its numpy restatement (tests/raygen_reference.py) and with the oracle's
// vo_primary_ray without a GPU.  A program of its own (tests/test_raygen_cpu.py builds it with g++ -ffp-contract=off, and once
// more with -fsanitize=address,undefined):
//     raygen_host IN OUT
// IN:  any number of records: vrt_ray_camera (108 bytes), int32 W, H.
// OUT: per record int32 rc (raygen_consts_of's: 0 ok, 1 unknown model, 2 bad tan_half / half_width, 3 degenerate basis) and,
//      when rc == 0, origins then dirs, W * H x 3 float32 each, ray py * W + px for pixel (px, py).
#include <cstdio>
#include <vector>

#include "../../include/vrt.h"
#include "../../voxel-raytracing_amd/csrc/vrt_raygen.h"

using namespace vrt;

static bool get(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
static bool put(FILE* f, const void* p, size_t n) { return n == 0 || fwrite(p, 1, n, f) == n; }

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: raygen_host IN OUT\n"); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "raygen_host: cannot open a file\n"); return 2; }
    static_assert(sizeof(vrt_ray_camera) == 108, "vrt_ray_camera layout");
    vrt_ray_camera cam;
    while (get(in, &cam, sizeof cam)) {
        int32_t wh[2];
        if (!get(in, wh, sizeof wh)) { fprintf(stderr, "raygen_host: short record\n"); return 2; }
        const int32_t W = wh[0], H = wh[1];
        if (W < 1 || H < 1 || W > 32768 || H > 32768) { fprintf(stderr, "raygen_host: bad size\n"); return 2; }
        RayCamConsts k;
        const int32_t rc = raygen_consts_of(cam, W, H, k);
        if (!put(out, &rc, 4)) return 2;
        if (rc != 0) continue;
        std::vector<float> col(2 * (size_t)W), row(2 * (size_t)H);
        if (k.model == VRT_CAMERA_PANORAMA) panorama_tables(W, H, col.data(), row.data());
        const size_t n = (size_t)W * (size_t)H;
        std::vector<float> o(3 * n), d(3 * n);
        for (int32_t py = 0; py < H; py++)
            for (int32_t px = 0; px < W; px++) {
                f3 ro, rd;
                camera_ray(k, col.data(), row.data(), px, py, ro, rd);
                const size_t i = ((size_t)py * (size_t)W + (size_t)px) * 3;
                o[i] = ro.x; o[i + 1] = ro.y; o[i + 2] = ro.z;
                d[i] = rd.x; d[i + 1] = rd.y; d[i + 2] = rd.z;
            }
        if (!put(out, o.data(), o.size() * 4) || !put(out, d.data(), d.size() * 4)) return 2;
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 2;
}
