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

// lane -> pixel.  span: role k of the span at (x0, py0) owns its rows 2k and 2k + 1; otherwise the 8x8 block at (x0, py0).
// (the terms in front of the lane's are wave-uniform: the choice costs no vector instruction)
VRT_HD void span_pixel(bool span, uint32_t x0, uint32_t py0, uint32_t role, uint32_t lane, int& px, int& py)
{
    const uint32_t mask = span ? 31u : 7u, sh = span ? 5u : 3u;
    px = (int)(x0 + (lane & mask));
    py = (int)(py0 + (span ? 2u * role : 0u) + (lane >> sh));
}

} // namespace vrt
