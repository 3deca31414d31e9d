// span_host.cpp -- TEST HELPER: the span rule of K1's sky waves (csrc/vrt_span.h) compiled for the host.  Built on demand by
// tests/test_sky_span_cpu.py with g++; never linked into libvrt_hip.so.
#include <cstdint>
#include "../../voxel-raytracing_amd/csrc/vrt_span.h"

using namespace vrt;

extern "C" {

// Every span of a W x H frame that lies inside its width, every block row, the 4 x 64 (role, lane) pairs: counts[py * W + px]
// is incremented for every pair with py < H.  Returns the number of pairs that left their span (px outside its 32 columns, py
// outside the block row's 8 rows, or px >= W).
int64_t span_cover(int W, int H, uint32_t* counts)
{
    int64_t outside = 0;
    for (uint32_t py0 = 0; py0 < (uint32_t)H; py0 += 8u)
        for (uint32_t col8 = 0; col8 * 8u < (uint32_t)W; col8++) {
            const uint32_t x0 = span_x0(col8);
            if (!span_in_frame(x0, (uint32_t)W)) continue;
            for (uint32_t lane = 0; lane < 64u; lane++) {
                int px, py;
                span_pixel(true, x0, py0, span_role(col8), lane, px, py);
                if (px < (int)x0 || px >= (int)x0 + 32 || py < (int)py0 || py >= (int)py0 + 8 || px >= W) { outside++; continue; }
                if (py < H) counts[(size_t)py * (size_t)W + (size_t)px]++;
            }
        }
    return outside;
}

// lane -> pixel of the per-block assignment (span = false): out[lane] = px | py << 16
void block_pixels(uint32_t px0, uint32_t py0, uint32_t* out)
{
    for (uint32_t lane = 0; lane < 64u; lane++) {
        int px, py;
        span_pixel(false, px0, py0, span_role(px0 >> 3), lane, px, py);
        out[lane] = (uint32_t)px | ((uint32_t)py << 16);
    }
}

// n cases: four tags each; out: 1 byte each
void span_eligible_cases(int n, const uint32_t* tags, const uint32_t* tag_all, const uint32_t* tile_gen, const uint32_t* box,
                         const uint32_t* x0, const uint32_t* py0, const uint32_t* W, unsigned char* out)
{
    for (int i = 0; i < n; i++)
        out[i] = span_eligible(tags[4 * i], tags[4 * i + 1], tags[4 * i + 2], tags[4 * i + 3], tag_all[i], tile_gen[i], box[i], x0[i], py0[i], W[i]) ? 1 : 0;
}

// What the wave of block column col8 decides, the way k_primary forms it: its span's four tags out of one tag row of tags_x
// words (the block's own where the span is cut by the frame's edge), then the rule.  out: one byte per block column.
void span_verdict_row(const uint32_t* tag_row, uint32_t tags_x, uint32_t tag_all, uint32_t tile_gen, uint32_t box, uint32_t py0, uint32_t W,
                      unsigned char* out)
{
    for (uint32_t col8 = 0; col8 < tags_x; col8++) {
        const uint32_t x0 = span_x0(col8);
        const bool in = span_in_frame(x0, W);
        const uint32_t first = in ? col8 - span_role(col8) : col8, step = in ? 1u : 0u;
        out[col8] = span_eligible(tag_row[first], tag_row[first + step], tag_row[first + 2u * step], tag_row[first + 3u * step], tag_all, tile_gen,
                                  box, x0, py0, W) ? 1 : 0;
    }
}

} // extern "C"
