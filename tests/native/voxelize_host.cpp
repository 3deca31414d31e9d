// Host build of csrc/vrt_voxelize.h for the tests (tests/voxelize_native.py): the header's predicates one by one, and the whole
// voxelization restated single-threaded with the header's own pieces -- the triangles' clipped boxes, the row and lane tests, the
// crossing count by division, the toggle mask and its scan -- as the kernels run them.
// With -DVOXELIZE_MAIN it is a stand-alone program that runs the range-edge cases (vertices at -65536 and 131072, bounds at both
// ends of a 4096-voxel axis) and prints one line per case; it is built with -fsanitize=signed-integer-overflow,address.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../voxel-raytracing_amd/csrc/vrt_voxelize.h"

using namespace vrt;

extern "C" int vox_meets_c(const int32_t tri[9], int32_t x, int32_t y, int32_t z)
{
    VoxTri T;
    vox_tri_setup(tri, tri + 3, tri + 6, T);
    return vox_meets(T, x, y, z) ? 1 : 0;
}

extern "C" int vox_flips_c(const int32_t tri[9], int32_t x, int32_t y, int32_t z)
{
    VoxTri T;
    vox_tri_setup(tri, tri + 3, tri + 6, T);
    return vox_flips(T, x, y, z) ? 1 : 0;
}

extern "C" void vox_axis_span_c(int32_t m, int32_t M, int32_t out[2]) { vox_axis_span(m, M, &out[0], &out[1]); }

extern "C" uint32_t vox_cross_count_c(const int32_t tri[9], int32_t x0, uint32_t size_x, int32_t y, int32_t z)
{
    VoxTri T;
    vox_tri_setup(tri, tri + 3, tri + 6, T);
    const int s = vox_cross_sign(T);
    return s == 0 ? 0u : vox_cross_count(T, s, x0, size_x, vox_centre(y), vox_centre(z));
}

// cover: size[0] * size[1] * size[2] bytes, x fastest, 1 = covered.  Returns 0, or 1 when an argument is refused.
// candidates (may be NULL): the candidate voxels and columns tested.
extern "C" int vox_cover_c(const int32_t* vertices, uint32_t nv, const uint32_t* triangles, uint32_t nt, uint32_t fill, const int32_t clo[3],
                           const uint32_t csize[3], uint8_t* cover, uint64_t* candidates)
{
    if (nt < 1u || nt > VRT_VOXELIZE_MAX_TRIANGLES || nv < 1u || nv > VRT_VOXELIZE_MAX_VERTICES) return 1;
    if (!vox_job_ok(0, 1u, 0u, fill, csize) || !vox_sides_ok(csize)) return 1;
    for (size_t i = 0; i < (size_t)nv * 3u; i++) if (!vox_coord_ok(vertices[i])) return 1;
    for (size_t i = 0; i < (size_t)nt * 3u; i++) if (triangles[i] >= nv) return 1;
    const size_t rows = (size_t)csize[1] * csize[2];
    const uint32_t wpr = vox_cover_words(csize[0]), tw = vox_toggle_words(csize[0]);
    std::vector<uint64_t> cmask(rows * wpr, 0), toggle((fill & VRT_VOXELIZE_FILL_SOLID) ? rows * tw : 0, 0);
    uint64_t cand = 0;
    for (uint32_t t = 0; t < nt; t++) {
        VoxTri T;
        int32_t lo[3], hi[3];
        vox_tri_setup(vertices + 3u * (size_t)triangles[3u * t], vertices + 3u * (size_t)triangles[3u * t + 1u], vertices + 3u * (size_t)triangles[3u * t + 2u], T);
        if ((fill & VRT_VOXELIZE_FILL_SURFACE) && vox_tri_box(T, false, clo, csize, lo, hi)) {
            for (int32_t z = lo[2]; z <= hi[2]; z++) for (int32_t y = lo[1]; y <= hi[1]; y++) {
                cand += (uint64_t)(hi[0] - lo[0] + 1);
                if (!vox_row_meets(T, vox_centre(y), vox_centre(z))) continue;
                const size_t row = vox_row_index((uint32_t)(y - clo[1]), (uint32_t)(z - clo[2]), csize);
                for (int32_t x = lo[0]; x <= hi[0]; x++)
                    if (vox_lane_meets(T, vox_centre(x), vox_centre(y), vox_centre(z))) {
                        const uint32_t bx = (uint32_t)(x - clo[0]);
                        cmask[row * wpr + (bx >> 6)] |= 1ull << (bx & 63u);
                    }
            }
        }
        if ((fill & VRT_VOXELIZE_FILL_SOLID) && vox_tri_box(T, true, clo, csize, lo, hi)) {
            const int s = vox_cross_sign(T);
            for (int32_t z = lo[2]; z <= hi[2]; z++) for (int32_t y = lo[1]; y <= hi[1]; y++) {
                cand++;
                if (!vox_column_inside(T, s, vox_centre(y), vox_centre(z))) continue;
                const uint32_t k = vox_cross_count(T, s, clo[0], csize[0], vox_centre(y), vox_centre(z));
                if (k != 0u) toggle[vox_row_index((uint32_t)(y - clo[1]), (uint32_t)(z - clo[2]), csize) * tw + (k >> 6)] ^= 1ull << (k & 63u);
            }
        }
    }
    if (fill & VRT_VOXELIZE_FILL_SOLID)
        for (size_t row = 0; row < rows; row++) {
            uint64_t carry = 0;
            for (uint32_t w = tw; w-- > 0u;) {
                const uint64_t in = vox_scan_word(toggle[row * tw + w], &carry);
                if (w < wpr) cmask[row * wpr + w] |= in & vox_word_valid(w, csize[0]);
            }
        }
    for (size_t row = 0; row < rows; row++)
        for (uint32_t bx = 0; bx < csize[0]; bx++) cover[row * csize[0] + bx] = (uint8_t)((cmask[row * wpr + (bx >> 6)] >> (bx & 63u)) & 1ull);
    if (candidates) *candidates = cand;
    return 0;
}

#ifdef VOXELIZE_MAIN
// The range-edge cases (tests/voxelize_native.py has the same list and holds the printed lines to Python integers)
static const int32_t kLo = VRT_VOXELIZE_COORD_MIN, kHi = VRT_VOXELIZE_COORD_MAX;
static const int32_t kCases[][9] = {
    {kLo, kLo, kLo, kHi, kHi, kHi, kHi, kLo, kHi},
    {kLo, kHi, kLo, kHi, kLo, kHi, kLo, kLo, kHi},
    {kHi, kLo, kLo, kLo, kHi, kLo, kLo, kLo, kHi},
    {kLo, kLo, kHi, kHi, kHi, kLo, kLo, kHi, kLo},
    {kLo, 200, 131, kHi, 260, 75, 17, kHi, kLo},
    {kLo, kLo, kLo, kHi, kHi, kHi, kHi, kHi, kHi},      // a segment, corner to corner
    {kHi, kHi, kHi, kHi, kHi, kHi, kHi, kHi, kHi},      // a point
};

int main()
{
    const int32_t corners[2][3] = {{0, 0, 0}, {4064, 4064, 4064}};
    const uint32_t size[3] = {32, 32, 32}, tri[3] = {0, 1, 2};
    std::vector<uint8_t> cover(32 * 32 * 32);
    for (size_t k = 0; k < sizeof kCases / sizeof kCases[0]; k++)
        for (int c = 0; c < 2; c++)
            for (uint32_t fill = 1; fill <= 3; fill++) {
                if (vox_cover_c(kCases[k], 3, tri, 1, fill, corners[c], size, cover.data(), nullptr) != 0) { std::printf("case %zu refused\n", k); return 1; }
                uint64_t n = 0, sum = 0;
                for (size_t i = 0; i < cover.size(); i++) if (cover[i]) { n++; sum += i * i; }
                std::printf("%zu %d %u %llu %llu\n", k, c, fill, (unsigned long long)n, (unsigned long long)sum);
            }
    return 0;
}
#endif
