// verdict_host.cpp -- TEST HELPER: the byte k_block_verdicts stores per block (csrc/vrt_span.h block_verdict_byte, fed through
// verdict_tag as the kernel feeds it), compiled for the host next to what k_primary's preamble worked out per wave (span_verdict +
// span_decide over one four-word fetch): that is the independent form.  The comparison with block_skips / span_eligible over
// the frame's own tag words checks the feeding (verdict_tag, the own tag's select, cut spans) -- the byte is written in terms
// of those two functions, so for the rule itself it proves little.  And the buffer's layout (verdict_pitch, verdict_offset,
// verdict_word, verdict_shift).  k_block_verdicts' own row -> pixel-row arithmetic is not compiled here: the GPU image tests carry it.
// Built on demand by tests/test_block_verdicts_cpu.py with g++; never linked into libvrt_hip.so.
#include <cstdint>
#include <vector>
#include "../../voxel-raytracing_amd/csrc/vrt_span.h"

using namespace vrt;

namespace {

// the wave's own decision, as the preamble formed it: one four-word fetch at the span's first block.  bit 0: skip, bit 1: span.
uint32_t decide_wave(const uint32_t* tg, uint32_t tags_x, uint32_t tags_per_frame, uint32_t row8, uint32_t col8, bool flag, uint32_t W,
                     uint32_t tile_gen, uint32_t box, uint32_t py0)
{
    const bool span_w = flag && span_in_frame(span_x0(col8), W);
    const uint32_t* w = tg + span_fetch_first(row8, col8, tags_x);
    const uint32_t v = span_verdict(w[0], w[1], w[2], w[3], span_fetch_own(col8, tags_x), span_w && tags_x != 0u, span_w, tg[tags_per_frame - 1u], tile_gen);
    return span_decide(v, box, col8 * 8u, py0);
}

// ... and by the definitions: the block's own tag for `skip`, the four of its span for `span`
uint32_t decide_defs(const uint32_t* tg, uint32_t tags_x, uint32_t tags_per_frame, uint32_t row8, uint32_t col8, bool flag, uint32_t W,
                     uint32_t tile_gen, uint32_t box, uint32_t py0)
{
    const uint32_t tag_all = tg[tags_per_frame - 1u];
    const uint32_t own = tags_x ? tg[row8 * tags_x + col8] : tg[0];
    const bool skip = block_skips(box, col8 * 8u, py0, own != tile_gen && tag_all != tile_gen);
    bool span = false;
    if (flag && span_in_frame(span_x0(col8), W)) {
        // (inside the frame's width all four blocks exist)
        const uint32_t* s = tags_x ? tg + row8 * tags_x + (col8 & ~3u) : nullptr;
        span = tags_x ? span_eligible(s[0], s[1], s[2], s[3], tag_all, tile_gen, box, span_x0(col8), py0, W)
                      : span_eligible(own, own, own, own, tag_all, tile_gen, box, span_x0(col8), py0, W);
    }
    return (skip ? 1u : 0u) | (span ? 2u : 0u);
}

// the byte, from the words the kernel reads
uint32_t decide_byte(const uint32_t* tg, uint32_t tags_x, uint32_t tags_per_frame, uint32_t row8, uint32_t col8, bool flag, uint32_t W,
                     uint32_t tile_gen, uint32_t box, uint32_t py0)
{
    const uint32_t tag_all = tg[tags_per_frame - 1u];
    uint32_t t[4];
    for (uint32_t j = 0; j < 4u; j++) t[j] = verdict_tag(tg + row8 * tags_x, (col8 & ~3u) + j, tags_x, tag_all, tile_gen);
    return block_verdict_byte(t[0], t[1], t[2], t[3], col8, flag, W, tag_all, tile_gen, box, py0);
}

} // namespace

extern "C" {

// One frame of width W (tags_x = ceil(W / 8) words per tag row, two tag rows, the frame's word behind them) or, with_tags = 0,
// the layout of a launch without tags (one word per frame).  Every block column of the second tag row (every role; whole spans
// and the span the right edge cuts), every pattern of the tags of its span, the frame's word set or not, the launch's span path
// on or off.  The words a pattern does not reach (the other row, the next frame, the spare words) hold tile_gen when poison is
// set.  Returns the number of cases in which the byte differs from the wave's decision or from the definitions; *cases: how
// many were compared; *seen: OR of 1 << byte over all cases.
int64_t verdict_compare(uint32_t W, int with_tags, uint32_t box, uint32_t py0, int poison, int64_t* cases, uint32_t* seen)
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
                    std::vector<uint32_t> tg(2u * tpf + 3u, poison ? gen : stale);
                    if (with_tags) {
                        for (uint32_t c = 0; c < tags_x; c++) tg[tags_x + c] = stale;
                        const uint32_t s0 = col8 & ~3u;
                        for (uint32_t j = 0; j < 4u && s0 + j < tags_x; j++) tg[tags_x + s0 + j] = ((pat >> j) & 1u) ? gen : stale;
                        tg[tpf - 1u] = all ? gen : stale;
                    } else {
                        tg[0] = (pat & 1u) ? gen : stale;            // (real launches hold tile_gen here; both are compared)
                    }
                    const uint32_t a = decide_wave(tg.data(), tags_x, tpf, row8, col8, flag != 0, W, gen, box, py0);
                    const uint32_t d = decide_defs(tg.data(), tags_x, tpf, row8, col8, flag != 0, W, gen, box, py0);
                    const uint32_t b = decide_byte(tg.data(), tags_x, tpf, row8, col8, flag != 0, W, gen, box, py0);
                    if (a != b || d != b || b > 3u) bad++;
                    (*cases)++;
                    *seen |= 1u << b;
                }
    return bad;
}

// The layout for a launch of n_frames frames of blocks_x x blocks_y blocks: every block has a byte of its own inside
// pitch * blocks_y * n_frames bytes, the word of a block is 4-byte aligned and holds the bytes of the (up to) four blocks of
// its span at bits 0, 8, 16, 24 in role order and of nobody else.  Returns the number of violations.
int64_t verdict_layout_errors(uint32_t blocks_x, uint32_t blocks_y, uint32_t n_frames)
{
    const uint32_t pitch = verdict_pitch(blocks_x);
    const uint64_t total = (uint64_t)pitch * blocks_y * n_frames;
    int64_t bad = 0;
    if (pitch % 4u != 0u || pitch < blocks_x || pitch >= blocks_x + 4u) bad++;
    std::vector<uint32_t> owner((size_t)total, 0xFFFFFFFFu);
    for (uint32_t f = 0; f < n_frames; f++)
        for (uint32_t r = 0; r < blocks_y; r++)
            for (uint32_t c = 0; c < blocks_x; c++) {
                const uint32_t o = verdict_offset(r, c, f, n_frames, pitch), w = verdict_word(r, c, f, n_frames, pitch);
                if (o >= total || w % 4u != 0u || o < w || 8u * (o - w) != verdict_shift(span_role(c))) { bad++; continue; }
                if (owner[o] != 0xFFFFFFFFu) bad++;
                owner[o] = (f * blocks_y + r) * blocks_x + (c & ~3u);      // (the span the byte belongs to)
            }
    // no word holds bytes of two spans
    for (uint64_t w = 0; w + 3u < total; w += 4u) {
        uint32_t first = 0xFFFFFFFFu;
        for (uint32_t j = 0; j < 4u; j++) {
            const uint32_t o = owner[(size_t)(w + j)];
            if (o == 0xFFFFFFFFu) continue;
            if (first == 0xFFFFFFFFu) first = o;
            else if (o != first) bad++;
        }
    }
    return bad;
}

uint32_t verdict_pitch_of(uint32_t blocks_x) { return verdict_pitch(blocks_x); }

} // extern "C"
