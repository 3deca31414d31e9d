// faces_host.cpp -- csrc/vrt_faces.h built for the host: the records of a box of a dense volume, made the way the kernels make them
// (per direction and segment of 64 lanes: exposed, continues the lane below, starts, lengths), single-threaded.  The tests hold it
// against tests/faces_reference.py; tools/exp_faces.py times it as the route vrt_scene_list_faces replaces.  With -DFACES_MAIN it is a
// program of its own (built with the sanitizers by the tests): a few generated volumes, one line per box and flag set.
#include <cstdio>
#include <vector>

#include "../../voxel-raytracing_amd/csrc/vrt_faces.h"

using namespace vrt;

namespace {

uint32_t voxel_at(const uint8_t* vol, const int32_t dim[3], const int32_t p[3])
{
    return vol[(size_t)p[0] + ((size_t)p[1] + (size_t)p[2] * (size_t)dim[1]) * (size_t)dim[0]];
}

} // namespace

extern "C" {

// -> the number of records; counts[d] always; the first min(total, capacity) records are written
uint64_t faces_list_c(const uint8_t* vol, const int32_t dim[3], const int32_t lo[3], const uint32_t size[3], uint32_t flags, uint64_t* records,
                      uint64_t capacity, uint64_t counts[6])
{
    uint64_t total = 0;
    for (uint32_t d = 0; d < VRT_FACES_DIRECTIONS; d++) {
        counts[d] = 0;
        const uint32_t nseg = face_segments(d, size);
        for (uint32_t g = 0; g < nseg; g++) {
            uint32_t b[64][3], id[64];
            bool exposed[64];
            for (uint32_t lane = 0; lane < 64u; lane++) {
                exposed[lane] = false;
                id[lane] = 0;
                if (!face_segment_voxel(d, g, lane, size, &b[lane][0], &b[lane][1], &b[lane][2])) continue;
                const int32_t own[3] = {lo[0] + (int32_t)b[lane][0], lo[1] + (int32_t)b[lane][1], lo[2] + (int32_t)b[lane][2]};
                const int32_t rel[3] = {(int32_t)b[lane][0], (int32_t)b[lane][1], (int32_t)b[lane][2]};
                int32_t p[3];
                id[lane] = voxel_at(vol, dim, own);
                exposed[lane] = id[lane] != 0u && (!face_neighbour_reads(d, rel, lo, size, dim, flags, p) || voxel_at(vol, dim, p) == 0u);
            }
            for (uint32_t lane = 0; lane < 64u; lane++) {
                if (!exposed[lane]) continue;
                const bool runs = (flags & VRT_FACES_FLAG_RUNS) != 0u;
                if (runs && lane != 0u && exposed[lane - 1u] && id[lane - 1u] == id[lane]) continue;      // continues the lane below
                uint32_t length = 1;
                while (runs && lane + length < 64u && exposed[lane + length] && id[lane + length] == id[lane]) length++;
                if (total < capacity) records[total] = face_record(b[lane][0], b[lane][1], b[lane][2], id[lane], length, d);
                total++;
                counts[d]++;
            }
        }
    }
    return total;
}

uint64_t faces_order_key_c(uint32_t d, uint32_t bx, uint32_t by, uint32_t bz, const uint32_t size[3]) { return face_order_key(d, bx, by, bz, size); }
uint64_t faces_record_c(uint32_t bx, uint32_t by, uint32_t bz, uint32_t id, uint32_t length, uint32_t d) { return face_record(bx, by, bz, id, length, d); }
int faces_record_valid_c(uint64_t r) { return face_record_valid(r) ? 1 : 0; }
void faces_quad_corner_c(uint64_t r, uint32_t k, uint32_t c[3]) { face_quad_corner(r, k, c); }

} // extern "C"

#if defined(FACES_MAIN)
// volumes of a linear congruential generator the tests restate: s = s * 1664525 + 1013904223 (mod 2^32) per voxel, x fastest;
// the voxel is empty when s >> 31, else its id is 1 + (s >> 8) % 3
int main()
{
    const int32_t dims[3][3] = {{70, 6, 5}, {5, 131, 4}, {9, 9, 9}};
    for (int v = 0; v < 3; v++) {
        const int32_t* dim = dims[v];
        std::vector<uint8_t> vol((size_t)dim[0] * dim[1] * dim[2]);
        uint32_t s = 12345u + (uint32_t)v;
        for (uint8_t& id : vol) {
            s = s * 1664525u + 1013904223u;
            id = (s >> 31) ? 0u : (uint8_t)(1u + (s >> 8) % 3u);
        }
        const int32_t los[2][3] = {{0, 0, 0}, {1, 1, 1}};
        for (int k = 0; k < 2; k++) {
            const int32_t* lo = los[k];
            const uint32_t size[3] = {(uint32_t)(dim[0] - 2 * lo[0]), (uint32_t)(dim[1] - 2 * lo[1]), (uint32_t)(dim[2] - 2 * lo[2])};
            for (uint32_t flags = 0; flags < 4u; flags++) {
                uint64_t counts[6];
                const uint64_t n = faces_list_c(vol.data(), dim, lo, size, flags, nullptr, 0, counts);
                std::vector<uint64_t> rec((size_t)n);
                if (faces_list_c(vol.data(), dim, lo, size, flags, rec.data(), n, counts) != n) return 1;
                uint64_t sum = 0;
                for (size_t i = 0; i < rec.size(); i++) {
                    if (!face_record_valid(rec[i])) return 2;
                    sum = (sum * 31u + rec[i]) & 0xFFFFFFFFFFFFull;
                }
                printf("%d %d %u %llu %llu %llu %llu %llu %llu %llu\n", v, k, flags, (unsigned long long)counts[0], (unsigned long long)counts[1],
                       (unsigned long long)counts[2], (unsigned long long)counts[3], (unsigned long long)counts[4], (unsigned long long)counts[5],
                       (unsigned long long)sum);
            }
        }
    }
    return 0;
}
#endif
