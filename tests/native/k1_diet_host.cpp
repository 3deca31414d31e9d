// k1_diet_host.cpp -- TEST HELPER: what k_primary's preamble was restated as (csrc/vrt_span.h span_verdict / span_decide),
// compiled for the host next to the form it replaced; and the identity behind the one-axis hit distance (csrc/vrt_spec.h one_axis_len_ok).
// Built on demand by tests/test_k1_diet_cpu.py with g++; never linked into libvrt_hip.so.
#include <cstdint>
#include <cmath>
#include <vector>
#include "../../voxel-raytracing_amd/csrc/vrt_span.h"

using namespace vrt;

namespace {

// The decision as k_primary formed it before: four single-word fetches (the block's own four times over where the span is cut or
// the launch has no span path; the frame's one word without tags), the select chain, span_untagged, block_skips twice.
// tg: the frame's tags.  Returns bit 0: skip, bit 1: span.
uint32_t decide_old(const uint32_t* tg, uint32_t tags_x, uint32_t tags_per_frame, uint32_t row8, uint32_t col8, bool flag, uint32_t W,
                    uint32_t tile_gen, uint32_t box, uint32_t py0)
{
    const bool span_w = flag && span_in_frame(span_x0(col8), W);
    const uint32_t own = row8 * tags_x + (tags_x ? col8 : 0u);
    const uint32_t first = (span_w && tags_x) ? own - span_role(col8) : own, step = (span_w && tags_x) ? 1u : 0u;
    const uint32_t st0 = tg[first], st1 = tg[first + step], st2 = tg[first + 2u * step], st3 = tg[first + 3u * step];
    const uint32_t k = own - first;
    const uint32_t tag = k == 0u ? st0 : (k == 1u ? st1 : (k == 2u ? st2 : st3));
    const uint32_t tag_all = tg[tags_per_frame - 1u];
    const uint32_t px0 = col8 * 8u;
    const bool span = span_w && block_skips(box, px0 & ~31u, py0, span_untagged(st0, st1, st2, st3, tag_all, tile_gen));
    const bool skip = block_skips(box, px0, py0, tag != tile_gen && tag_all != tile_gen);
    return (skip ? 1u : 0u) | (span ? 2u : 0u);
}

// ... and as it forms it now: one four-word fetch at the span's first block
uint32_t decide_new(const uint32_t* tg, uint32_t tags_x, uint32_t tags_per_frame, uint32_t row8, uint32_t col8, bool flag, uint32_t W,
                    uint32_t tile_gen, uint32_t box, uint32_t py0)
{
    const bool span_w = flag && span_in_frame(span_x0(col8), W);
    const uint32_t* w = tg + span_fetch_first(row8, col8, tags_x);
    const uint32_t v = span_verdict(w[0], w[1], w[2], w[3], span_fetch_own(col8, tags_x), span_w && tags_x != 0u, span_w, tg[tags_per_frame - 1u], tile_gen);
    return span_decide(v, box, col8 * 8u, py0);
}

} // namespace

extern "C" {

// One frame of width W (tags_x = ceil(W / 8) words per tag row, two tag rows, the frame's word behind them) or, with_tags = 0,
// the layout of a launch without tags (one word per frame).  Every block column of the second tag row, every pattern of the
// tags of its span (the words the pattern does not reach hold tile_gen when poison is set: the next row, the spare words),
// the frame's word set or not, the launch's span path on or off: old and new decision compared.  box, py0: the caller's.
// Returns the number of cases that differ; *cases: how many were compared; *seen: OR of 1 << decision over all cases.
int64_t span_compare(uint32_t W, int with_tags, uint32_t box, uint32_t py0, int poison, int64_t* cases, uint32_t* seen)
{
    const uint32_t gen = 7u, stale = 6u;
    const uint32_t tags_x = with_tags ? (W + 7u) / 8u : 0u, tags_y = with_tags ? 2u : 0u, tpf = tags_x * tags_y + 1u;
    const uint32_t row8 = with_tags ? 1u : 0u;
    int64_t bad = 0;
    *cases = 0; *seen = 0u;
    const uint32_t ncol = (W + 7u) / 8u;
    for (uint32_t col8 = 0; col8 < ncol; col8++)
        for (uint32_t pat = 0; pat < 16u; pat++)
            for (int all = 0; all < 2; all++)
                for (int flag = 0; flag < 2; flag++) {
                    // two frames' worth of words + the three spare ones; the case lives in frame 0
                    std::vector<uint32_t> tg(2u * tpf + 3u, poison ? gen : stale);
                    if (with_tags) {
                        for (uint32_t c = 0; c < tags_x; c++) tg[c] = poison ? gen : stale;                     // (row 0: somebody else's)
                        for (uint32_t c = 0; c < tags_x; c++) tg[tags_x + c] = stale;
                        const uint32_t s0 = col8 & ~3u;
                        for (uint32_t j = 0; j < 4u && s0 + j < tags_x; j++) tg[tags_x + s0 + j] = ((pat >> j) & 1u) ? gen : stale;
                        tg[tpf - 1u] = all ? gen : stale;
                    } else {
                        tg[0] = (pat & 1u) ? gen : stale;            // (real launches hold tile_gen here; both are compared)
                    }
                    const uint32_t a = decide_old(tg.data(), tags_x, tpf, row8, col8, flag != 0, W, gen, box, py0);
                    const uint32_t b = decide_new(tg.data(), tags_x, tpf, row8, col8, flag != 0, W, gen, box, py0);
                    if (a != b) bad++;
                    (*cases)++;
                    *seen |= 1u << a;
                }
    return bad;
}

// every binary32 x = +-(1 + m * 2^-23) * 2^e, m = 0 .. 2^23 - 1: how many have len3((x, 0, 0)) != |x| (len3: the spec's own, the
// products and sums in float, the IEEE square root); *refused: how many of them one_axis_len_ok turns away for mask 1
int64_t one_axis_mismatches(int e, int64_t* refused)
{
    int64_t bad = 0;
    *refused = 0;
    for (uint32_t m = 0; m < (1u << 23); m++) {
        const float x = ldexpf(1.0f + (float)m * 0x1p-23f, e);
        for (int sgn = 0; sgn < 2; sgn++) {
            const float v = sgn ? -x : x;
            if (!(len3(mk3(v, 0.0f, 0.0f)) == x) || !(len3(mk3(0.0f, v, 0.0f)) == x) || !(len3(mk3(0.0f, 0.0f, v)) == x)) bad++;
            if (!one_axis_len_ok(1u, v)) (*refused)++;
        }
    }
    return bad;
}

int one_axis_ok(uint32_t mask, float x) { return one_axis_len_ok(mask, x) ? 1 : 0; }
float one_axis_len3(float x) { return len3(mk3(0.0f, x, 0.0f)); }

} // extern "C"
