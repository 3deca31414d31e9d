"""tests/scene_reference.py (what a fresh scene build must contain, in numpy) held against literal brute force, and its comparers
against single-byte and single-bit slips; no GPU.
  * clearance: a cube grown voxel by voxel with explicit bounds, on volumes with sides 1..10, all eight octants, caps below and
    above the volume's side;
  * brick_fine: the 24^3 window built explicitly, for bricks at a corner, on a face and inside a volume;
  * the point-wise reference of the 832^3 test against the whole-field one, its box test against the literal slice test;
  * the comparers name the field / word / bit group and the coordinates of a slip;
  * the three-pass builder of tests/native/traverse_host.cpp (the fields the host march tests walk through) gives the same
    clearance."""
import ctypes as C
import itertools

import numpy as np
import pytest

import extents_common
import scene_reference as R
from test_traverse_host import th                                 # noqa: F401  (the fixture that builds and loads the library)


def brute_clearance(vol, o, cap):
    D, H, W = vol.shape
    solid = (vol != 0).tolist()
    sx, sy, sz = R.signs(o)
    out = np.zeros(vol.shape, np.int32)
    for z, y, x in itertools.product(range(D), range(H), range(W)):
        k = 0
        while k < cap:
            ok = True                                             # does the cube of side k + 1 still hold?  Only its new shell is looked at
            for c, b, a in itertools.product(range(k + 1), repeat=3):
                if max(a, b, c) != k:
                    continue
                qx, qy, qz = x + a * sx, y + b * sy, z + c * sz
                if qx < 0 or qx >= W or qy < 0 or qy >= H or qz < 0 or qz >= D or solid[qz][qy][qx]:
                    ok = False
                    break
            if not ok:
                break
            k += 1
        out[z, y, x] = k
    return out


def small_volumes():
    rng = np.random.default_rng(7)
    vols = [("empty 4x3x5", np.zeros((5, 3, 4), np.uint8)), ("full 3x3x3", np.full((3, 3, 3), 7, np.uint8)),
            ("one voxel", np.zeros((1, 1, 1), np.uint8)), ("one solid voxel", np.ones((1, 1, 1), np.uint8)),
            ("a dimension of 1", (rng.random((6, 1, 9)) < 0.1).astype(np.uint8)), ("a line", (rng.random((1, 1, 10)) < 0.2).astype(np.uint8)),
            ("empty 10x2x2", np.zeros((2, 2, 10), np.uint8)), ("empty 6x6x6", np.zeros((6, 6, 6), np.uint8))]
    for k in range(8):
        d, h, w = (int(v) for v in rng.integers(1, 8, 3))
        vols.append((f"random {w}x{h}x{d}", ((rng.random((d, h, w)) < (0.03, 0.15, 0.4)[k % 3]) * rng.integers(1, 255, (d, h, w))).astype(np.uint8)))
    vols.append(("sparse 10x9x8", (rng.random((8, 9, 10)) < 0.01).astype(np.uint8)))
    return vols


def test_clearance_is_the_brute_force_cube():
    sides = set()
    for name, vol in small_volumes():
        sides.update(vol.shape)
        for cap in (3, 127) if vol.size > 200 else (1, 2, 3, 16, 127):
            for o in range(8):
                got, exp = R.clearance(vol, o, cap), brute_clearance(vol, o, cap)
                assert got.shape == exp.shape and (got == exp).all(), (name, cap, o, np.argwhere(got != exp)[:3].tolist())
    assert sides == set(range(1, 11))


def test_open_cells_is_the_box_to_the_corner():
    rng = np.random.default_rng(3)
    for shape, p in (((5, 6, 7), 0.02), ((1, 9, 4), 0.05), ((6, 6, 6), 0.0), ((3, 3, 3), 1.0)):
        vol = (rng.random(shape) < p).astype(np.uint8)
        D, H, W = shape
        for o in range(8):
            sx, sy, sz = R.signs(o)
            got = R.open_cells(vol, o)
            for z, y, x in itertools.product(range(D), range(H), range(W)):
                box = vol[slice(z, D) if sz > 0 else slice(0, z + 1), slice(y, H) if sy > 0 else slice(0, y + 1), slice(x, W) if sx > 0 else slice(0, x + 1)]
                assert bool(got[z, y, x]) == (not box.any()), (shape, o, x, y, z)


def brute_fine_of_brick(vol, bx, by, bz):
    """[o, 512] of one brick from its 24^3 window, built explicitly: outside the volume solid; beyond the window solid"""
    D, H, W = vol.shape
    win = np.ones((24, 24, 24), bool)
    for wz, wy, wx in itertools.product(range(24), repeat=3):
        x, y, z = bx * 8 - 8 + wx, by * 8 - 8 + wy, bz * 8 - 8 + wz
        if 0 <= x < W and 0 <= y < H and 0 <= z < D:
            win[wz, wy, wx] = vol[z, y, x] != 0
    out = np.zeros((8, 512), np.uint8)
    for o in range(8):
        sx, sy, sz = R.signs(o)
        for lz, ly, lx in itertools.product(range(8), repeat=3):
            x, y, z = 8 + lx, 8 + ly, 8 + lz
            k = 0
            while k < R.FINE_CAP:
                x0, x1 = (x, x + k + 1) if sx > 0 else (x - k, x + 1)
                y0, y1 = (y, y + k + 1) if sy > 0 else (y - k, y + 1)
                z0, z1 = (z, z + k + 1) if sz > 0 else (z - k, z + 1)
                if min(x0, y0, z0) < 0 or max(x1, y1, z1) > 24 or win[z0:z1, y0:y1, x0:x1].any():
                    break
                k += 1
            out[o, lx + 8 * ly + 64 * lz] = k
    return out


def test_brick_fine_is_the_clearance_inside_the_window():
    assert R.FINE_CAP == 16 and R.BRICK_CAP == 16 and R.DF_CAP >= 64
    rng = np.random.default_rng(11)
    vol = ((rng.random((32, 40, 48)) < 0.003) * rng.integers(1, 255, (32, 40, 48))).astype(np.uint8)      # 6 x 5 x 4 bricks
    vol[31, 39, 47] = 5                                           # a brick whose only voxel is the volume's far corner
    vol[8:32, 8:32, 8:40] = 0
    vol[16, 16, 16] = 9                                           # brick (2, 2, 2): one voxel in its corner, empty neighbours
    ref = R.brick_fine_by_brick(vol)
    seen = set()
    for bx, by, bz in ((0, 0, 0), (5, 4, 3), (2, 0, 1), (0, 2, 2), (2, 2, 2), (3, 2, 1)):                   # corners, faces, interior
        exp = brute_fine_of_brick(vol, bx, by, bz)
        assert (ref[bz, by, bx] == exp).all(), (bx, by, bz, np.argwhere(ref[bz, by, bx] != exp)[:3].tolist())
        if vol[bz * 8:bz * 8 + 8, by * 8:by * 8 + 8, bx * 8:bx * 8 + 8].any():
            seen.update(exp.reshape(-1).tolist())
    # solid voxels, short ones, and the window's 9..15.  16 cannot occur: only a cube that starts in a corner of the brick and
    # runs inwards along all three axes has a window of 16, and it covers the whole brick, which holds a solid voxel
    assert set(range(0, 16)) <= seen and 16 not in seen, sorted(seen)


def test_point_reference_is_the_field_reference():
    rng = np.random.default_rng(5)
    vol = (rng.random((21, 17, 30)) < 0.004).astype(np.uint8)
    vol[8:16, 8:16, 16:24] = 3
    D, H, W = vol.shape
    pr = R.PointReference(vol)
    for _ in range(300):                                          # the box test is the slice test
        lo = [int(rng.integers(0, n)) for n in (W, H, D)]
        hi = [int(rng.integers(l + 1, n + 1)) for l, n in zip(lo, (W, H, D))]
        assert pr.box_any(lo, hi) == bool(vol[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]].any()), (lo, hi)
    for cap in (5, 127):
        for o in range(8):
            c, op = R.clearance(vol, o, cap), R.open_cells(vol, o)
            pts = [(0, 0, 0), (W - 1, H - 1, D - 1), (W - 1, 0, 0), (0, H - 1, D - 1)] + [tuple(int(rng.integers(0, n)) for n in (W, H, D)) for _ in range(150)]
            for x, y, z in pts:
                assert pr.clearance((x, y, z), o, cap) == c[z, y, x], (cap, o, x, y, z)
                assert pr.open((x, y, z), o) == bool(op[z, y, x]), (o, x, y, z)


def test_pyramid_and_cells_by_hand():
    vol = np.zeros((9, 6, 21), np.uint8)                          # W 21, H 6, D 9: 6 x 2 x 3 cells, 2 x 1 x 1 words above, 1 on top
    vol[0, 0, 0] = 1; vol[8, 5, 20] = 2; vol[2, 3, 17] = 3
    o1, o2, o3 = R.pyramid(vol)
    assert o1.shape == (36,) and o2.shape == (2,) and o3.shape == (2,)         # OCC3: one word and its padding
    exp1 = np.zeros(36, np.uint64)
    exp1[0] = 1                                                   # voxel (0, 0, 0): cell 0, bit 0
    exp1[5 + 6 * (1 + 2 * 2)] = np.uint64(1) << np.uint64(0 | (1 << 2) | (0 << 4))        # (20, 5, 8): cell (5, 1, 2), bit (0, 1, 0)
    exp1[4 + 6 * (0 + 2 * 0)] = np.uint64(1) << np.uint64(1 | (3 << 2) | (2 << 4))        # (17, 3, 2): cell (4, 0, 0), bit (1, 3, 2)
    assert (o1 == exp1).all()
    # level 2: cells (0,0,0) -> word 0 bit 0; (5,1,2) -> word 1, bit (1, 1, 2); (4,0,0) -> word 1, bit (0, 0, 0)
    assert int(o2[0]) == 1 and int(o2[1]) == (1 << (1 | (1 << 2) | (2 << 4))) | 1
    assert int(o3[0]) == 0b11 and int(o3[1]) == 0
    assert R.cells(vol).tolist() == sorted([0, 5 | (1 << 10) | (2 << 20), 4])


# ---- the comparers see what they must -----------------------------------------------------------------------------------------

def test_df_comparer_names_field_and_coordinates():
    rng = np.random.default_rng(2)
    W, H, D = 9, 6, 5
    vol = ((rng.random((D, H, W)) < 0.05) * rng.integers(1, 255, (D, H, W))).astype(np.uint8)
    vol[2, 3, 4] = 77
    ref = R.dense_df_bytes(vol, True)
    ndf, n = R.df_field_bytes(W, H, D), (W + 2) * (H + 2) * (D + 2)
    assert ndf == 768 and n == 616 and ref.size == 9 * ndf + 256 and ref[9 * ndf] == 0xFF and not ref[9 * ndf + 1:].any()
    assert R.diff_df(ref.copy(), ref, (W, H, D)) is None
    assert "holds" in R.diff_df(ref[:-1], ref, (W, H, D))
    idx = lambda f, x, y, z: f * ndf + (x + 1) + ((y + 1) + (z + 1) * (H + 2)) * (W + 2)
    z, y, x = (int(v[0]) for v in np.nonzero(R.dense_fields(vol, True)[5] > 1))
    slips = [(idx(5, x, y, z), +1, f"field 5 x {x} y {y} z {z}:"), (idx(5, x, y, z), -1, f"field 5 x {x} y {y} z {z}:"),
             (idx(0, 0, 0, 0), +1, "field 0 x 0 y 0 z 0:"), (idx(7, W - 1, H - 1, D - 1), +1, f"field 7 x {W - 1} y {H - 1} z {D - 1}:"),
             (idx(3, -1, 2, 2), +1, "field 3 x -1 y 2 z 2 (border)"), (idx(6, W, H, D), +1, f"field 6 x {W} y {H} z {D} (border)"),
             (idx(2, 4, -1, 0), +1, "field 2 x 4 y -1 z 0 (border)"), (idx(8, 0, 0, D), +1, f"field 8 x 0 y 0 z {D} (border)"),
             (1 * ndf + n, +1, "field 1 rounding tail byte 0"), (8 * ndf - 1, +1, f"field 7 rounding tail byte {ndf - n - 1}"),
             (9 * ndf - 1, +1, f"field 8 rounding tail byte {ndf - n - 1}"),
             (9 * ndf, -1, "the 0xFF byte behind field 8"), (9 * ndf + 1, +1, "tail byte 1 behind the 0xFF byte"), (9 * ndf + 255, +1, "tail byte 255"),
             (idx(8, 4, 3, 2), +1, "field 8 x 4 y 3 z 2:")]
    for i, delta, where in slips:
        bad = ref.copy()
        bad[i] = (int(bad[i]) + delta) & 0xFF
        msg = R.diff_df(bad, ref, (W, H, D), "case")
        assert msg is not None and where in msg and f"first at {i}," in msg and f"{int(bad[i])} != {int(ref[i])}" in msg, (i, where, msg)
    assert int(ref[idx(8, 4, 3, 2)]) == 77


def test_pyramid_and_cell_comparers_name_word_and_bit():
    rng = np.random.default_rng(4)
    vol = (rng.random((9, 22, 70)) < 0.02).astype(np.uint8)       # 18 x 6 x 3 cells, 5 x 2 x 1 words, 2 x 1 x 1
    levels = R.pyramid(vol)
    assert [l.size for l in levels] == [18 * 6 * 3, 10, 2]
    for k, (name, lv) in enumerate(zip(("OCC1", "OCC2", "OCC3"), levels)):
        n = R.level_dims((70, 22, 9), k + 1)
        assert R.diff_words(lv.copy(), lv, name, n) is None
        w = lv.size - 1 if k == 0 else 1
        bad = lv.copy()
        bad[w] ^= np.uint64(1) << np.uint64(2 | (1 << 2) | (3 << 4))
        msg = R.diff_words(bad, lv, name, n, "case")
        assert name in msg and f"word x {w % n[0]} y {w // n[0] % n[1]} z {w // (n[0] * n[1])}" in msg and "bit 54 (x 2 y 1 z 3)" in msg, msg
    bad = levels[2].copy()                                        # 2 words: no padding.  A level with padding:
    l3 = R.pyramid(np.ones((4, 4, 4), np.uint8))[2]
    assert l3.tolist() == [1, 0]
    bad = l3.copy(); bad[1] = 1
    assert "the padding word" in R.diff_words(bad, l3, "OCC3", (1, 1, 1))
    cl = R.cells(vol)
    assert R.diff_cells(cl[::-1].copy(), cl) is None              # in no particular order
    assert "x 3 y 1 z 2" in R.diff_cells(np.append(cl, np.uint32(3 | (1 << 10) | (2 << 20))), cl) or (3 | (1 << 10) | (2 << 20)) in cl.tolist()
    gone = int(cl[5])
    assert f"x {gone & 1023} y {gone >> 10 & 1023} z {gone >> 20}" in R.diff_cells(np.delete(cl, 5), cl)


def test_entry_comparer_names_brick_and_bit_group():
    grid = np.zeros((4, 3, 5), np.uint32)                         # 5 x 3 x 4 bricks
    grid[1, 1, 2] = 1; grid[3, 2, 4] = 2
    nb = (5, 3, 4)
    ref = R.brick_entries(grid, True)
    assert ref.shape == (7 * 5 * 6,)
    at = lambda x, y, z: (x + 1) + ((y + 1) + (z + 1) * 5) * 7
    assert int(ref[0]) == 0xFFFFFF and int(ref[at(2, 1, 1)]) == 1 and int(ref[at(4, 2, 3)]) == 2          # border and occupied: nothing but the pointer
    e = int(ref[at(0, 0, 0)])                                     # towards +x +y +z it sees brick (2, 1, 1): not open, clear for 2; towards -x -y -z open, 1 to the wall
    assert e & 0xFFFFFF == 0 and (e >> 24) & 0xFF == 0x7F and (e >> 32) & 0xF == 1 and (e >> 60) & 0xF == 2
    assert R.diff_entries(ref.copy(), ref, nb) is None and R.diff_entries(ref.copy(), ref, nb, slots=2) is None
    assert not (R.brick_entries(grid, False) >> np.uint64(24) & np.uint64(0xFF)).any()
    i = at(3, 0, 2)
    for bit, group in ((24 + 3, "open bit of octant 3"), (24 + 7, "open bit of octant 7"), (32, "coarse clearance of octant 0"),
                       (32 + 4 * 5 + 2, "coarse clearance of octant 5"), (63, "coarse clearance of octant 7")):
        bad = ref.copy()
        bad[i] ^= np.uint64(1) << np.uint64(bit)
        for slots in (None, 2):
            msg = R.diff_entries(bad, ref, nb, slots, "case")
            assert msg and group in msg and f"padded index {i} (brick x 3 y 0 z 2)" in msg, msg
    for j, val, where in ((i, 1, "brick x 3 y 0 z 2"), (at(2, 1, 1), 0, "brick x 2 y 1 z 1"), (0, 0, "brick x -1 y -1 z -1"), (at(2, 1, 1), 5, "brick x 2 y 1 z 1")):
        bad = ref.copy()
        bad[j] = (bad[j] & ~R.PTR_MASK) | np.uint64(val)
        msg = R.diff_entries(bad, ref, nb, None, "case")
        assert msg and "pointer" in msg and where in msg, msg
        if val != 5:
            assert "pointer" in R.diff_entries(bad, ref, nb, 2, "case")
    moved = ref.copy()                                            # a reserved scene may hold a brick in another slot ...
    moved[at(2, 1, 1)] = 2; moved[at(4, 2, 3)] = 1
    assert R.diff_entries(moved, ref, nb, 2) is None and "pointer" in R.diff_entries(moved, ref, nb)
    moved[at(4, 2, 3)] = 3                                        # ... but not past the pool, and no two in one
    assert "pointer" in R.diff_entries(moved, ref, nb, 2) and R.diff_entries(moved, ref, nb, 3) is None
    moved[at(4, 2, 3)] = 2
    assert "brick x 2 y 1 z 1" in R.diff_entries(moved, ref, nb, 2)


def test_brick_byte_comparer_names_slot_octant_and_voxel():
    rng = np.random.default_rng(6)
    vol = np.zeros((16, 24, 32), np.uint8)
    vol[8:16, 8:16, 16:24] = rng.integers(0, 3, (8, 8, 8))
    vol[3, 20, 1] = 9
    nb = (4, 3, 2)
    grid = np.zeros((2, 3, 4), np.uint32)
    grid[1, 1, 2] = 2; grid[0, 2, 0] = 1                          # the pool in another order than the bricks lie in the volume
    ent = R.brick_entries(grid, True)
    by_brick = R.brick_fine_by_brick(vol)
    pool = np.stack([R.to_bricks(vol)[0, 2, 0], R.to_bricks(vol)[1, 1, 2]])
    fine = np.stack([by_brick[0, 2, 0], by_brick[1, 1, 2]])
    assert R.diff_brick_bytes(ent, pool, fine, vol, nb) is None
    bad = fine.copy(); bad[1, 6, 3 + 8 * 2 + 64 * 5] += 1
    msg = R.diff_brick_bytes(ent, pool, bad, vol, nb, "case")
    assert "BFINE slot 1 (brick x 2 y 1 z 1)" in msg and "octant 6 voxel x 3 y 2 z 5" in msg, msg
    bad = pool.copy(); bad[0, 7 + 8 * 7] ^= 1
    assert "BPOOL slot 0 (brick x 0 y 2 z 0) voxel x 7 y 7 z 0" in R.diff_brick_bytes(ent, bad, fine, vol, nb)
    assert "BFINE" in R.diff_brick_bytes(ent, pool, fine[::-1].copy(), vol, nb)
    wrong = ent.copy(); wrong[(0 + 1) + ((0 + 1) + (0 + 1) * 5) * 6] |= np.uint64(2)
    assert "brick x 0 y 0 z 0 is empty" in R.diff_brick_bytes(wrong, pool, fine, vol, nb)


# ---- the host builder the march tests walk through ---------------------------------------------------------------------------

def test_the_host_builder_gives_the_same_clearance(th):             # noqa: F811
    th.thb_octant_clearance.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    th.thb_octant_clearance.restype = None
    rng = np.random.default_rng(9)
    vols = [np.zeros((20, 30, 140), np.uint8), (rng.random((24, 32, 40)) < 0.01).astype(np.uint8), (rng.random((7, 1, 19)) < 0.1).astype(np.uint8),
            (rng.random((5, 6, 7)) < 0.5).astype(np.uint8), np.ones((3, 4, 5), np.uint8)]
    for vol in vols:
        D, H, W = vol.shape
        for cap in (16, 127):
            for o in range(8):
                out = np.empty(vol.shape, np.uint8)
                th.thb_octant_clearance(np.ascontiguousarray(vol).ctypes.data, W, H, D, o, cap, out.ctypes.data)
                exp = R.clearance(vol, o, cap)
                assert (out == exp).all(), (vol.shape, cap, o, np.argwhere(out != exp)[:3].tolist())


# ---- the definition at the longest axis a scene may have ------------------------------------------------------------------------

NEEDLES = extents_common.NEEDLES + extents_common.RAGGED + extents_common.LINES      # the needle rows of tests/test_gpu_scene_build.py's DIMS


@pytest.mark.parametrize("dims", NEEDLES, ids=lambda d: "x".join(str(v) for v in d))
def test_the_definition_at_a_4096_axis(dims):
    """the needles of tests/test_gpu_scene_build.py (content of tests/extents_common.py; on the lines sparse voxels and both ends): clearance
    and open cells against the literal cube and box at the corners, along both ends of the long axis, at the clearance's cap and at
    random points; the pyramid and the cell list against a literal loop over the solid voxels -- cell coordinates 0 and 1023 occur,
    and 1023 is the largest"""
    W, H, D = dims
    a = int(np.argmax(dims))
    L = dims[a]
    rng = np.random.default_rng(L + a)
    if min(dims) > 1:
        vol = extents_common.needle_volume(dims)
    else:
        vol = ((rng.random((D, H, W)) < 0.004) * rng.integers(1, 256, (D, H, W))).astype(np.uint8)
        vol.reshape(-1)[[0, L - 1]] = 7
    solid = vol != 0
    pts = [((W - 1) * (k & 1), (H - 1) * (k >> 1 & 1), (D - 1) * (k >> 2)) for k in range(8)]
    for along in list(range(0, 8)) + list(range(L - 8, L)) + [100, 130, 227, 228, L - 130, L // 2 + 599, L // 2 + 602] + [int(v) for v in rng.integers(0, L, 40)]:
        p = [int(rng.integers(0, n)) for n in dims]
        p[a] = along
        pts.append(tuple(p))
    capped = False
    for o in range(8):
        sx, sy, sz = R.signs(o)
        clear, op = R.clearance(vol, o, R.DF_CAP), R.open_cells(vol, o)
        capped |= bool((clear == R.DF_CAP).any())
        for x, y, z in pts:
            k = 0
            while k < R.DF_CAP:                                   # the cube of side k + 1 from (x, y, z) towards the octant
                x0, x1 = (x, x + k + 1) if sx > 0 else (x - k, x + 1)
                y0, y1 = (y, y + k + 1) if sy > 0 else (y - k, y + 1)
                z0, z1 = (z, z + k + 1) if sz > 0 else (z - k, z + 1)
                if min(x0, y0, z0) < 0 or x1 > W or y1 > H or z1 > D or solid[z0:z1, y0:y1, x0:x1].any():
                    break
                k += 1
            assert clear[z, y, x] == k, (o, x, y, z, int(clear[z, y, x]), k)
            box = solid[slice(z, D) if sz > 0 else slice(0, z + 1), slice(y, H) if sy > 0 else slice(0, y + 1), slice(x, W) if sx > 0 else slice(0, x + 1)]
            assert bool(op[z, y, x]) == (not box.any()), (o, x, y, z)
    assert capped == (min(dims) >= R.DF_CAP)                      # a cube's side is the needle's width at most
    zs, ys, xs = np.nonzero(solid)
    keys = sorted({(int(x) >> 2) | (int(y) >> 2) << 10 | (int(z) >> 2) << 20 for x, y, z in zip(xs, ys, zs)})
    assert R.cells(vol).tolist() == keys
    coord = [k >> (10 * a) & 1023 for k in keys]
    assert min(coord) == 0 and max(coord) == 1023
    n1 = R.level_dims(dims, 1)
    exp1 = np.zeros(n1[0] * n1[1] * n1[2], np.uint64)
    for x, y, z in zip(xs.tolist(), ys.tolist(), zs.tolist()):
        exp1[(x >> 2) + n1[0] * ((y >> 2) + n1[1] * (z >> 2))] |= np.uint64(1) << np.uint64((x & 3) | (y & 3) << 2 | (z & 3) << 4)
    assert (R.pyramid(vol)[0] == exp1).all()
