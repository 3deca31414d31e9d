"""csrc/vrt_morph.h on the host.  First the reference proves what the header states about itself (tests/morph_reference.py: the
closed form over the ball's offsets equals r unit steps; which operations can add and which can remove; opening and closing are
idempotent; erosion and dilation are dual; bounds inside the volume give the whole-volume result restricted to them).  Then the
header's tiled algorithm -- row-word masks over the domain, extended blocks, r steps a tile (tests/native/morph_host.cpp) -- is held
to that reference bit for bit, and a program of its own runs it under the sanitizers."""
import itertools

import numpy as np
import pytest

from morph_common import blobs
import morph_native as N
import morph_reference as M

OPS = (M.DILATE, M.ERODE, M.OPEN, M.CLOSE, M.HOLLOW)


@pytest.mark.parametrize("conn,r", list(itertools.product((6, 26), (1, 2, 8))))
def test_closed_form_equals_unit_steps(conn, r):
    dims = (11, 9, 10) if r == 8 else (17, 12, 14)
    vol = blobs(dims, 10 * conn + r, block=2 if r < 8 else 5)
    for op, border in itertools.product(OPS, (False, True)):
        a = M.result_set(vol, op, conn, r, border, "closed")
        b = M.result_set(vol, op, conn, r, border, "steps")
        assert (a == b).all(), (op, conn, r, border)
    n = len(M.ball(conn, r))
    assert n == ((2 * r + 1) ** 3 if conn == 26 else (2 * r + 1) * (2 * r * r + 2 * r + 3) // 3)       # the cube; the octahedron


def test_known_counts_of_a_single_voxel():
    vol = np.zeros((19, 19, 19), np.uint8)
    vol[9, 9, 9] = 5
    for how in ("steps", "closed"):                                              # the octahedron and the cube, the voxel itself included
        assert int((M.morph(vol, M.DILATE, 8, 6, 7, how=how)[0] != 0).sum()) == 833 and M.morph(vol, M.DILATE, 8, 6, 7, how=how)[1]["added"] == 832
        assert int((M.morph(vol, M.DILATE, 8, 26, 7, how=how)[0] != 0).sum()) == 17 ** 3


@pytest.mark.parametrize("conn,r,border", list(itertools.product((6, 26), (1, 2), (False, True))))
def test_what_the_operations_can_do(conn, r, border):
    vol = blobs((20, 15, 17), 3 * conn + r)
    whole = {}
    for op in OPS:
        out, res = M.morph(vol, op, r, conn, 201, None, border)
        whole[op] = out
        if op in (M.ERODE, M.OPEN, M.HOLLOW):
            assert res["added"] == 0 and ((out != 0) <= (vol != 0)).all()
        else:
            assert res["removed"] == 0 and ((vol != 0) <= (out != 0)).all()
        assert res["added"] + res["removed"] == res["changed"] == int((out != vol).sum())
        assert ((out == vol) | (out == 0) | (out == 201)).all()                     # never recoloured
        if op in (M.OPEN, M.CLOSE):                                                  # idempotent over whole-volume bounds
            again, res2 = M.morph(out, op, r, conn, 202, None, border)
            assert res2["changed"] == 0 and (again == out).all(), (op, res2)
    # duality: ERODE with the border solid is the complement of DILATE of the complement with the border empty
    comp = (vol == 0).astype(np.uint8)
    assert ((M.morph(vol, M.ERODE, r, conn, 0, None, True)[0] != 0) == (M.morph(comp, M.DILATE, r, conn, 1, None, False)[0] == 0)).all()
    # the halo: bounds inside the volume give the whole-volume result restricted to them, and touch nothing else
    lo, size = (4, 3, 5), (9, 8, 7)
    inb = np.zeros(vol.shape, bool)
    inb[5:12, 3:11, 4:13] = True
    for op in OPS:
        part, res = M.morph(vol, op, r, conn, 201, (lo, size), border)
        assert (part[inb] == whole[op][inb]).all() and (part[~inb] == vol[~inb]).all(), op
    # ... and the result reads nothing beyond the halo: what lies farther from the bounds than that does not matter
    for op in OPS:
        h = M.halo(op, r)
        far = vol.copy()
        keep = np.zeros(vol.shape, bool)
        keep[max(0, 5 - h):12 + h, max(0, 3 - h):11 + h, max(0, 4 - h):13 + h] = True
        far[~keep] = np.where(far[~keep] != 0, 0, 9)
        a, b = M.morph(vol, op, r, conn, 201, (lo, size), border)[0], M.morph(far, op, r, conn, 201, (lo, size), border)[0]
        assert (a[inb] == b[inb]).all(), op


def test_argument_rules():
    ok = (4, 4, 4)
    assert N.args_ok(M.DILATE, 6, 1, 0, 1, ok) and N.args_ok(M.HOLLOW, 26, 8, 3, 0, ok) and N.args_ok(M.ERODE, 6, 8, 0, 0, (1 << 30, 1, 1))
    for op, conn, r, flags, vid, size in ((5, 6, 1, 0, 1, ok), (-1, 6, 1, 0, 1, ok), (M.ERODE, 18, 1, 0, 0, ok), (M.ERODE, 0, 1, 0, 0, ok), (M.ERODE, 6, 0, 0, 0, ok),
                                          (M.ERODE, 6, 9, 0, 0, ok), (M.ERODE, 6, -1, 0, 0, ok), (M.ERODE, 6, 1, 4, 0, ok), (M.DILATE, 6, 1, 0, 0, ok), (M.CLOSE, 26, 1, 0, 0, ok),
                                          (M.CLOSE, 26, 1, 0, 256, ok), (M.ERODE, 6, 1, 0, 0, (0, 4, 4)), (M.ERODE, 6, 1, 0, 0, (4, 4, (1 << 30) + 1))):
        assert not N.args_ok(op, conn, r, flags, vid, size) and not M.args_ok(op, conn, r, flags, vid, size), (op, conn, r, flags, vid, size)
    assert N.sides_ok((512, 512, 512)) and not N.sides_ok((513, 1, 1)) and not N.sides_ok((1, 1, 513))
    for op in OPS:
        assert [N.halo(op, r) for r in (1, 3, 8)] == [M.halo(op, r) for r in (1, 3, 8)]
    assert [N.phases(op) for op in OPS] == [[False], [True], [True, False], [False, True], [True]]
    for op, bit, old in itertools.product(OPS, (False, True), (0, 7)):
        in_r = (old != 0 and not bit) if op == M.HOLLOW else bit
        assert N.value(op, bit, old, 33) == (33 if in_r and old == 0 else 0 if not in_r and old != 0 else old)


def test_layout_against_python_integers():
    rng = np.random.default_rng(4)
    for clo, cs, h in (((0, 0, 0), (1, 1, 1), 1), ((3, 0, 9), (512, 512, 512), 16), ((5, 6, 7), (63, 9, 33), 8), ((0, 2, 0), (70, 45, 52), 3)):
        mlo, ms = N.domain(clo, cs, h)
        assert mlo == [c - h for c in clo] and ms == [c + 2 * h for c in cs] and max(ms) <= 544
        nw = -(-ms[0] // 32)
        assert N.row_words(ms[0]) == nw and N.mask_words(ms) == nw * ms[1] * ms[2]
        assert N.tiles(ms) == [-(-nw // 2), -(-ms[1] // 16), -(-ms[2] // 16)]
        for _ in range(30):
            m = [int(rng.integers(0, s)) for s in ms]
            assert N.word_index((m[0] >> 5, m[1], m[2]), ms) == (m[0] >> 5) + nw * (m[1] + ms[1] * m[2])
        assert N.word_index((nw - 1, ms[1] - 1, ms[2] - 1), ms) == N.mask_words(ms) - 1
    assert N.row_words(544) == 17 and N.mask_words((544, 544, 544)) * 4 == 17 * 4 * 544 * 544


def same(vol, op, r, conn, vid=201, bounds=None, border=False):
    exp_vol, exp = M.morph(vol, op, r, conn, vid, bounds, border)
    rc, got_vol, got = N.morph(vol, op, r, conn, vid, bounds, border)
    assert rc == 0 and got == exp, (op, r, conn, bounds, border, got, exp)
    assert (got_vol == exp_vol).all(), (op, r, conn, bounds, border)
    rc, kept, meas = N.morph(vol, op, r, conn, vid, bounds, border, measure=True)
    assert rc == 0 and (kept == vol).all() and meas == dict(M.ZERO, added=exp["added"], removed=exp["removed"])
    return exp_vol, exp


@pytest.mark.parametrize("conn,r", list(itertools.product((6, 26), (1, 2, 8))))
def test_tiled_algorithm_equals_the_reference(conn, r):
    # more than one tile along every axis, more than two row words, no side a multiple of anything
    vol = blobs((70, 21, 19), 7 * conn + r, block=4 if r < 8 else 9)
    for op, border in itertools.product(OPS, (False, True)):
        same(vol, op, r, conn, border=border)
    for op in OPS:
        same(vol, op, r, conn, bounds=((-4, 3, -2), (40, 9, 30)), border=True)          # clipped by three faces
        same(vol, op, r, conn, bounds=((31, 5, 4), (9, 9, 9)))                          # strictly inside


def test_row_word_edges_and_known_counts():
    vol = blobs((131, 9, 7), 5, block=3)
    for x0, x1 in itertools.product((63, 64, 65), repeat=2):
        for op in (M.DILATE, M.OPEN, M.HOLLOW):
            same(vol, op, 2, 26, bounds=((x0, 0, 0), (x1 + 1, 9, 7)))                   # x range x0 .. x0 + x1: starts and ends around the word edges
    for x0, x1 in itertools.product((63, 64, 65), repeat=2):
        if x1 > x0:
            same(vol, M.CLOSE, 1, 6, bounds=((x0, 1, 1), (x1 - x0, 5, 5)))
        same(vol, M.ERODE, 1, 6, bounds=((0, 0, 0), (x1, 9, 7)))
        same(vol, M.DILATE, 3, 6, bounds=((x0, 0, 0), (131 - x0, 9, 7)))
    one = np.zeros((19, 19, 19), np.uint8)
    one[9, 9, 9] = 5
    assert same(one, M.DILATE, 8, 6)[1]["added"] == 833 - 1 and same(one, M.DILATE, 8, 26)[1]["added"] == 17 ** 3 - 1
    assert same(one, M.HOLLOW, 1, 6)[1]["changed"] == 0 and same(one, M.OPEN, 1, 6)[1]["removed"] == 1


def test_random_small_volumes():
    rng = np.random.default_rng(12)
    for k in range(300):
        dims = tuple(int(v) for v in rng.integers(1, 14, 3))
        vol = blobs(dims, 1000 + k, p=float(rng.uniform(0.2, 0.9)), block=int(rng.integers(1, 4)))
        op, conn, r = int(rng.integers(0, 5)), (6, 26)[int(rng.integers(0, 2))], int(rng.integers(1, 4)) if k % 10 else 8
        lo = tuple(int(v) for v in rng.integers(-3, 6, 3))
        size = tuple(int(v) for v in rng.integers(1, 16, 3))
        same(vol, op, r, conn, bounds=None if k % 3 == 0 else (lo, size), border=bool(k % 2))


def test_clip_and_sides():
    vol = np.zeros((2, 3, 600), np.uint8)
    vol[:, :, 40:560] = 3
    assert N.morph(vol, M.ERODE, 1, bounds=((0, 0, 0), (513, 3, 2)))[0] == 1
    assert N.morph(vol, M.ERODE, 1, bounds=((-50, 0, 0), (563, 3, 2)))[0] == 1
    same(vol, M.ERODE, 1, 6, bounds=((-50, 0, 0), (562, 3, 2)), border=True)           # 512 after the clip
    same(vol, M.OPEN, 8, 26, bounds=((88, 0, 0), (512, 3, 2)), border=True)            # the domain is 544 long
    assert same(vol, M.DILATE, 2, 6, bounds=((700, 0, 0), (4, 4, 4)))[1] == M.ZERO     # wholly outside


def test_fuzz_program_under_asan_and_ubsan(tmp_path):
    """tests/native/morph_fuzz.cpp, a program of its own, with -fsanitize=address,undefined and no recovery: the tiled algorithm
    against the closed form, with bounds at the int32 edges; an overflow or a mask index out of range would end it"""
    import os
    import re
    import subprocess
    src = os.path.join(N.ROOT, "tests", "native", "morph_fuzz.cpp")
    exe = str(tmp_path / "morph_fuzz_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, src])
    for seed in ("1", "2"):
        r = subprocess.run([exe, seed, "60"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
        m = re.match(r"(\d+) calls, (\d+) voxels changed", r.stdout)
        assert m and int(m.group(1)) == 120 and int(m.group(2)) >= 120, r.stdout      # not vacuous: a voxel a call at the least, on average
