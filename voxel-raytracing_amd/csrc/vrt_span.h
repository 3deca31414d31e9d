// vrt_span.h -- the sky waves of an all-sky 32x8 span store whole rows (k_primary, vrt_device.hip).
//
// A wave of K1 traces one 8x8 block of pixels, lane l -> (l & 7, l >> 3): a store of a 4-byte plane touches eight 128-byte lines,
// 32 bytes of each.  For the waves that march that footprint is worth its price (a 16x4 block measured 3 % slower); a wave that
// only stores the miss pixel has no footprint to protect.  So where the four horizontally adjacent blocks of a SPAN -- 32x8
// pixels, 32-pixel aligned in x -- are ALL skip blocks (outside the frame's box rectangle, or none of them tagged), the four
// waves trade pixels among themselves: the wave of block k = col8 & 3 takes rows 2k and 2k + 1 of the span, lane l ->
// (l & 31, l >> 5), and every store of a 4-byte plane is two whole 128-byte rows.
//
// Nothing is shared between the waves and nobody does another wave's work: every wave of a span reads the same four tag words
// (they lie next to each other in one tag row) and the same box word (the rectangle is in units of 32 pixels), reaches the same
// verdict, and produces the miss pixel of whichever pixel a lane holds -- by the sky-texel fast path or, where some lane is not
// sure of its texel, the long way round: the four waves may take different ways and the picture is the same.
// tests/test_sky_span_cpu.py (through tests/native/span_host.cpp) checks that the (role, lane) pairs of a span hit each of its
// pixels exactly once and that the verdict does not depend on the role.
#pragma once

#include "vrt_spec.h"

namespace vrt {

// first pixel column of the span the block column col8 (in 8-pixel blocks) lies in
VRT_HD uint32_t span_x0(uint32_t col8) { return (col8 & ~3u) << 3; }
// the role of that block's wave within its span
VRT_HD uint32_t span_role(uint32_t col8) { return col8 & 3u; }

// the span lies wholly inside the frame's width (a span cut by the right edge runs block by block)
VRT_HD bool span_in_frame(uint32_t x0, uint32_t W) { return x0 + 32u <= W; }

// Is the block at (px0, py0) a skip block?  box: the frame's rectangle in units of 32 pixels, columns [b0, b1) x rows [b2, b3)
// as b0 | b1 << 8 | b2 << 16 | b3 << 24 (0xFF00FF00: the whole screen, nothing is known); untagged: neither the block's tag nor
// the frame's "the tags say nothing" word equals the launch's tile_gen.
VRT_HD bool block_skips(uint32_t box, uint32_t px0, uint32_t py0, bool untagged)
{
    const uint32_t bx = px0 >> 5, by = py0 >> 5;
    return box != 0xFF00FF00u && (bx < (box & 0xFFu) || bx >= ((box >> 8) & 0xFFu) || by < ((box >> 16) & 0xFFu) || by >= (box >> 24) || untagged);
}

// none of the span's four tags, nor the frame's word, says "trace"
VRT_HD bool span_untagged(uint32_t t0, uint32_t t1, uint32_t t2, uint32_t t3, uint32_t tag_all, uint32_t tile_gen)
{
    return t0 != tile_gen && t1 != tile_gen && t2 != tile_gen && t3 != tile_gen && tag_all != tile_gen;
}

// The span rule: every one of the four blocks of the span at (x0, py0) is a skip block and the span is not cut by the frame's
// right edge.  (The rectangle test is the same for the four blocks: x0 is a multiple of 32 and they share py0.)
VRT_HD bool span_eligible(uint32_t t0, uint32_t t1, uint32_t t2, uint32_t t3, uint32_t tag_all, uint32_t tile_gen, uint32_t box,
                          uint32_t x0, uint32_t py0, uint32_t W)
{
    return span_in_frame(x0, W) && block_skips(box, x0, py0, span_untagged(t0, t1, t2, t3, tag_all, tile_gen));
}

// ---- the same rule as k_primary reaches it: one fetch, one compare chain, one rectangle test ----
// (tests/test_k1_diet_cpu.py, through tests/native/k1_diet_host.cpp, proves that this form and the functions above agree for
// every tag pattern, box, role and width.)
//
// The four tags of a span are neighbours in one tag row, so ONE four-word fetch at the span's first block brings them all: a scalar
// load needs its address aligned to a word, not to its size, and the row pitch may be anything.  Where the span is cut by the
// frame's right edge the words past the row's end belong to the next row (after the last row: to the frame's "the tags say
// nothing" word, the next frame, or the three spare words the host allocates behind the last frame); in a launch without tags
// (tags_x = 0, one word per frame) words 1 - 3 are other frames'.  Neither is looked at: `wide` says whether all four words are
// this span's blocks, otherwise only the block's own counts.

// the word offset of the fetch within the frame's tags
VRT_HD uint32_t span_fetch_first(uint32_t row8, uint32_t col8, uint32_t tags_x) { return tags_x ? row8 * tags_x + (col8 & ~3u) : 0u; }
// which of the four fetched words is the block's own
VRT_HD uint32_t span_fetch_own(uint32_t col8, uint32_t tags_x) { return tags_x ? span_role(col8) : 0u; }

// bit 0: the block has no tag; bit 1: its span may take the span path (span_w: the launch has the path and the span lies inside
// the frame's width); bit 2: none of the span's blocks has a tag.  own: span_fetch_own; wide = span_w && tags_x != 0.
VRT_HD uint32_t span_verdict(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t own, bool wide, bool span_w, uint32_t tag_all,
                             uint32_t tile_gen)
{
    const uint32_t hits = (w0 == tile_gen ? 1u : 0u) | (w1 == tile_gen ? 2u : 0u) | (w2 == tile_gen ? 4u : 0u) | (w3 == tile_gen ? 8u : 0u);
    const uint32_t mine = 1u << own, seen = wide ? 15u : mine;
    const uint32_t v = ((hits & mine) ? 0u : 1u) | ((hits & seen) ? 0u : 4u);
    return (tag_all == tile_gen ? 0u : v) | (span_w ? 2u : 0u);
}

// the block at (px0, py0) lies outside the frame's box rectangle (the same answer for the four blocks of a span: the rectangle is
// in units of 32 pixels)
VRT_HD bool block_outside(uint32_t box, uint32_t px0, uint32_t py0)
{
    const uint32_t bx = px0 >> 5, by = py0 >> 5;
    // (bitwise: four compares and three ORs on the scalar unit, no branch)
    return (bool)((int)(bx < (box & 0xFFu)) | (int)(bx >= ((box >> 8) & 0xFFu)) | (int)(by < ((box >> 16) & 0xFFu)) | (int)(by >= (box >> 24)));
}

// What the wave does, from span_verdict's bits: bit 0: the block is a skip block (block_skips); bit 1: the span is eligible
// (span_eligible).  Outside the rectangle nobody has a tag that counts; without a rectangle nothing is known.
VRT_HD uint32_t span_decide(uint32_t verdict, uint32_t box, uint32_t px0, uint32_t py0)
{
    const uint32_t u = (verdict | (block_outside(box, px0, py0) ? 5u : 0u)) & (box != 0xFF00FF00u ? 7u : 0u);
    return (u & 1u) | ((u & 6u) == 6u ? 2u : 0u);
}

// lane -> pixel.  span: role k of the span at (x0, py0) owns its rows 2k and 2k + 1; otherwise the 8x8 block at (x0, py0).
// (the terms in front of the lane's are wave-uniform: the choice costs no vector instruction)
VRT_HD void span_pixel(bool span, uint32_t x0, uint32_t py0, uint32_t role, uint32_t lane, int& px, int& py)
{
    const uint32_t mask = span ? 31u : 7u, sh = span ? 5u : 3u;
    px = (int)(x0 + (lane & mask));
    py = (int)(py0 + (span ? 2u * role : 0u) + (lane >> sh));
}

} // namespace vrt
