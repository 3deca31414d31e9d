"""The span rule of K1's sky waves (csrc/vrt_span.h) on the CPU, with the header the kernel compiles: where the four 8x8 blocks of
a 32x8 span are all skip blocks, the wave of block k takes rows 2k and 2k + 1 of the span instead of its block.
  * the 4 x 64 (role, lane) pairs of every span inside the frame's width hit each of the span's pixels with py < H exactly once
    and nothing outside it, for ragged and full-size frames;
  * the rule says no whenever one of the four tags, or the frame's word, equals tile_gen, and whenever the span is cut by the
    frame's right edge;
  * the four waves of a span reach the same verdict from one tag row."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "span_host.cpp")
LIB = os.path.join(ROOT, "tests", "native", "libspan_host.so")
HDR = os.path.join(ROOT, "voxel-raytracing_amd", "csrc", "vrt_span.h")

WHOLE = 0xFF00FF00           # FrameSlot::box {0, 255, 0, 255}: nothing is known about the frame


@pytest.fixture(scope="module")
def span():
    if not os.path.exists(LIB) or any(os.path.getmtime(LIB) < os.path.getmtime(p) for p in (SRC, HDR)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", LIB, SRC])
    l = C.CDLL(LIB)
    l.span_cover.restype = C.c_int64
    l.span_cover.argtypes = [C.c_int, C.c_int, C.c_void_p]
    l.block_pixels.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p]
    l.span_eligible_cases.argtypes = [C.c_int] + [C.c_void_p] * 8
    l.span_verdict_row.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    return l


def _box(b0, b1, b2, b3):
    return b0 | (b1 << 8) | (b2 << 16) | (b3 << 24)


def eligible(l, tags, tag_all, tile_gen, box, x0, py0, W):
    n = len(tags)
    a = lambda v: np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.uint32), (n,)))
    tags = np.ascontiguousarray(tags, np.uint32)
    arrs = [a(tag_all), a(tile_gen), a(box), a(x0), a(py0), a(W)]
    out = np.zeros(n, np.uint8)
    l.span_eligible_cases(n, tags.ctypes.data, *[v.ctypes.data for v in arrs], out.ctypes.data)
    return out.astype(bool)


@pytest.mark.parametrize("H", [8, 9, 40, 1080])
@pytest.mark.parametrize("W", [32, 33, 63, 64, 72, 130, 1920])
def test_role_and_lane_hit_every_pixel_of_a_span_once(span, W, H):
    counts = np.zeros((H, W), np.uint32)
    assert span.span_cover(W, H, counts.ctypes.data) == 0
    inside = (W // 32) * 32                                     # the columns of the spans that are not cut by the right edge
    assert (counts[:, :inside] == 1).all()
    assert (counts[:, inside:] == 0).all()


def test_block_assignment_is_the_8x8_block(span):
    out = np.zeros(64, np.uint32)
    span.block_pixels(72, 40, out.ctypes.data)
    lane = np.arange(64)
    assert ((out & 0xFFFF) == 72 + (lane & 7)).all() and ((out >> 16) == 40 + (lane >> 3)).all()


def test_rule_says_no_for_a_tag_the_frames_word_and_the_right_edge(span):
    rng = np.random.default_rng(11)
    n = 4000
    gen = rng.integers(1, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    tags = rng.integers(0, 1 << 32, (n, 4), dtype=np.uint64).astype(np.uint32)
    tags[tags == gen[:, None]] ^= 1                             # no tag equals tile_gen ...
    tag_all = np.where(gen == 7, 8, 7).astype(np.uint32)
    box = _box(1, 3, 0, 2)                                      # columns [32, 96) x rows [0, 64)
    W = 256
    for x0 in (0, 32, 64, 96, 224):
        for py0 in (0, 8, 56, 64, 120):
            # ... so every span is eligible: outside the rectangle anyway, inside it because nothing is tagged
            assert eligible(span, tags, tag_all, gen, box, x0, py0, W).all()
            for k in range(4):                                  # one tagged block: never inside the rectangle, always outside it
                t = tags.copy(); t[:, k] = gen
                inside = 32 <= x0 < 96 and py0 < 64
                assert (eligible(span, t, tag_all, gen, box, x0, py0, W) == (not inside)).all()
            assert (eligible(span, tags, gen, gen, box, x0, py0, W) == (not (32 <= x0 < 96 and py0 < 64))).all()
            # a frame without a rectangle: nothing is skipped, tagged or not
            assert not eligible(span, tags, tag_all, gen, WHOLE, x0, py0, W).any()
    # a tag anywhere, or the frame's word, inside the rectangle: never eligible; the right edge: never eligible
    for k in range(4):
        t = tags.copy(); t[:, k] = gen
        assert not eligible(span, t, tag_all, gen, _box(0, 8, 0, 8), 64, 8, W).any()
    assert not eligible(span, tags, gen, gen, _box(0, 8, 0, 8), 64, 8, W).any()
    for Wc, x0 in ((33, 32), (63, 32), (72, 64), (130, 128), (255, 224), (31, 0)):
        assert not eligible(span, tags, tag_all, gen, box, x0, 200, Wc).any()        # (row 200: outside the rectangle)
        assert not eligible(span, tags, tag_all, gen, _box(0, 0, 0, 0), x0, 0, Wc).any()
    assert eligible(span, tags, tag_all, gen, box, 32, 200, 64).all()                # span_x0 + 32 == W is inside


def test_the_four_waves_of_a_span_agree(span):
    rng = np.random.default_rng(12)
    n_rows, some_yes, some_no = 3000, 0, 0
    for r in range(n_rows):
        W = int(rng.choice([32, 33, 63, 64, 72, 130, 200, 1920]))
        tags_x = (W + 7) // 8
        gen = int(rng.integers(1, 1 << 32))
        row = rng.integers(0, 1 << 32, tags_x, dtype=np.uint64).astype(np.uint32)
        row[row == gen] ^= 1
        row[rng.random(tags_x) < rng.choice([0.0, 0.05, 0.3])] = gen
        tag_all = gen if rng.random() < 0.05 else (gen ^ 0x55)
        box = WHOLE if rng.random() < 0.05 else _box(int(rng.integers(0, 4)), int(rng.integers(2, 62)), 0, int(rng.integers(1, 40)))
        py0 = int(rng.integers(0, 135)) * 8
        out = np.zeros(tags_x, np.uint8)
        span.span_verdict_row(row.ctypes.data, tags_x, tag_all, gen, box, py0, W, out.ctypes.data)
        for s in range(tags_x // 4 + 1):
            blk = out[4 * s:4 * s + 4]
            if 32 * s + 32 > W:
                assert not blk.any()                            # cut by the right edge (or not a whole span): block by block
                continue
            assert blk.all() or not blk.any(), (r, s, blk)
            # ... and it is the rule: every block of the span is a skip block
            b0, b1, b2, b3 = box & 0xFF, (box >> 8) & 0xFF, (box >> 16) & 0xFF, box >> 24
            outside = s < b0 or s >= b1 or (py0 >> 5) < b2 or (py0 >> 5) >= b3
            untagged = tag_all != gen and not (row[4 * s:4 * s + 4] == gen).any()
            want = box != WHOLE and (outside or untagged)
            assert bool(blk[0]) == want, (r, s)
            some_yes += want; some_no += not want
    assert some_yes > 1000 and some_no > 1000
