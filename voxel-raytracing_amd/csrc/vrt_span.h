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

// ---- the same rule made ONCE per launch: one byte per block (k_block_verdicts, vrt_device.hip) ----
// (tests/test_block_verdicts_cpu.py, through tests/native/verdict_host.cpp, proves that the byte is span_verdict + span_decide's
// answer, and block_skips / span_eligible's, for every tag pattern, role, box and width.)
//
// Everything above is a function of (frame, block) and known once the tags are made, yet every wave of k_primary works it out
// again on the scalar unit.  The primary-only kernels of table launches read it instead: bit 0: the block is a skip block (block_skips); bit 1: its
// span is eligible (span_eligible) and the launch has the span path.  The bytes lie in the launch's LOCAL block rows like the tags,
// rows padded to a multiple of four blocks: the four bytes of a span are one 4-byte-aligned word, which a wave fetches with one
// scalar load and takes its own byte from.

// Block row r of frame f of a launch of n_frames frames is row r * n_frames + f of the buffer: a wave finds its word from what the
// tile map holds (its frame, the launch's n_frames and block columns) and the launch needs no stride of its own in the kernel
// arguments -- the megakernels' argument block keeps its size and they their machine code.

// bytes per row of blocks_x blocks
VRT_HD uint32_t verdict_pitch(uint32_t blocks_x) { return (blocks_x + 3u) & ~3u; }
// byte offset of block (row8, col8) of frame `frame`
VRT_HD uint32_t verdict_offset(uint32_t row8, uint32_t col8, uint32_t frame, uint32_t n_frames, uint32_t pitch) { return (row8 * n_frames + frame) * pitch + col8; }
// the bit a block's byte starts at within its span's word, from its role (span_role(col8))
VRT_HD uint32_t verdict_shift(uint32_t role) { return role << 3; }
// ... and the byte offset of the word that holds the byte
VRT_HD uint32_t verdict_word(uint32_t row8, uint32_t col8, uint32_t frame, uint32_t n_frames, uint32_t pitch) { return verdict_offset(row8, col8 & ~3u, frame, n_frames, pitch); }

// The tag of block column c as the verdict pass sees it.  row: the block row's tags (tags_x of them).  A launch without tags
// (tags_x = 0) has the frame's one word, which holds tile_gen: nothing is untagged and the box alone decides.  A column the row
// does not have is part of a span the frame's right edge cuts, which is not eligible whatever its tags: a value that is no tag.
VRT_HD uint32_t verdict_tag(const uint32_t* row, uint32_t c, uint32_t tags_x, uint32_t tag_all, uint32_t tile_gen)
{
    return tags_x == 0u ? tag_all : (c < tags_x ? row[c] : ~tile_gen);
}

// The byte of the block at column col8 whose first pixel row is py0.  t0 .. t3: the tags of its span's four blocks (a block the
// frame does not have: any value -- such a span is cut and not eligible); span_path: the launch has the span path; W: the
// frame's width.
VRT_HD uint32_t block_verdict_byte(uint32_t t0, uint32_t t1, uint32_t t2, uint32_t t3, uint32_t col8, bool span_path, uint32_t W,
                                   uint32_t tag_all, uint32_t tile_gen, uint32_t box, uint32_t py0)
{
    const uint32_t own = span_role(col8);
    const uint32_t tag = own == 0u ? t0 : (own == 1u ? t1 : (own == 2u ? t2 : t3));
    const bool skip = block_skips(box, col8 << 3, py0, tag != tile_gen && tag_all != tile_gen);
    const bool span = span_path && span_eligible(t0, t1, t2, t3, tag_all, tile_gen, box, span_x0(col8), py0, W);
    return (skip ? 1u : 0u) | (span ? 2u : 0u);
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
