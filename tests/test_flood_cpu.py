"""csrc/vrt_flood.h on the host (tests/native/flood_host.cpp): the header's tiled algorithm -- masks, extended rows, tile steps,
wake-up flags, rounds -- run in forward, reverse and seeded-random tile order, and with every tile of a round blind to what the
round's other tiles gained, equals a plain breadth-first search (tests/flood_reference.py) bit for bit.  Also the argument rules,
the clip, the index functions against Python integers, the tile step and the loop bound."""
import itertools

import numpy as np
import pytest

import flood_common as fc
import flood_native as N
import flood_reference as F

ORDERS = ("forward", "reverse", "random", "stale")


def same(vol, seed, vid, match, conn, bounds=None, measure=False, orders=ORDERS):
    exp_vol, exp = F.flood(vol, seed, vid, match, conn, bounds, measure)
    for order in orders:
        rc, got_vol, got, rounds = N.flood(vol, seed, vid, match, conn, bounds, measure, order, rng=5)
        assert rc == 0 and got == exp, (order, got, exp)
        assert (got_vol == exp_vol).all(), order
        assert rounds >= 1 or exp["region"] == 0
    return exp_vol, exp


def test_argument_rules():
    ok = (4, 4, 4)
    assert N.args_ok(F.SAME, 6, 0, ok) and N.args_ok(F.SOLID, 26, F.MEASURE, ok) and N.args_ok(F.SAME, 6, 0, (1 << 30, 1, 1))
    for match, conn, flags, size in ((2, 6, 0, ok), (-1, 6, 0, ok), (F.SAME, 18, 0, ok), (F.SAME, 0, 0, ok), (F.SAME, 27, 0, ok), (F.SAME, 6, 2, ok),
                                     (F.SAME, 6, 3, ok), (F.SAME, 6, 0, (0, 4, 4)), (F.SAME, 6, 0, (4, 4, (1 << 30) + 1)), (F.SAME, 6, 0, (4, 0xFFFFFFFF, 4))):
        assert not N.args_ok(match, conn, flags, size) and not F.args_ok(match, conn, flags, size), (match, conn, flags, size)
    assert N.sides_ok((512, 512, 512)) and not N.sides_ok((513, 1, 1)) and not N.sides_ok((1, 1, 513))
    assert N.seed_inside((3, 4, 5), (3, 4, 5), (1, 1, 1)) and not N.seed_inside((4, 4, 5), (3, 4, 5), (1, 1, 1)) and not N.seed_inside((2, 4, 5), (3, 4, 5), (9, 9, 9))
    assert N.seed_inside((-(1 << 31), 0, 0), (-(1 << 31), 0, 0), (1, 1, 1)) is True
    for vid, sid in itertools.product((0, 1, 7, 255), repeat=2):
        assert N.passes(F.SAME, vid, sid) == (vid == sid) and N.passes(F.SOLID, vid, sid) == (vid != 0)


def test_index_functions_against_python_integers():
    rng = np.random.default_rng(3)
    for cs in ((1, 1, 1), (8, 8, 8), (9, 16, 17), (512, 512, 512), (70, 45, 52), (511, 3, 505)):
        nt = N.tiles(cs)
        assert nt == [-(-c // 8) for c in cs] and max(nt) <= 64
        assert N.round_bound(cs) == cs[0] * cs[1] * cs[2] + 1
        for _ in range(50):
            r = [int(rng.integers(0, c)) for c in cs]
            t = [v >> 3 for v in r]
            ti = t[0] + (t[1] + t[2] * nt[1]) * nt[0]
            assert N.tile_index(t, nt) == ti
            assert N.mask_byte(r, nt) == ti * 64 + (r[1] & 7) + 8 * (r[2] & 7) and N.mask_bit(r[0]) == r[0] & 7
        last = [c - 1 for c in cs]
        assert N.mask_byte(last, nt) < nt[0] * nt[1] * nt[2] * 64
    assert N.round_bound((512, 512, 512)) == 2 ** 27 + 1


def _mask_of(bits, nt):
    """bool [z, y, x] over the tiles' voxels -> the mask's bytes"""
    m = np.zeros(nt[0] * nt[1] * nt[2] * 64, np.uint8)
    for z, y, x in zip(*np.nonzero(bits)):
        m[N.mask_byte((x, y, z), nt)] |= 1 << (x & 7)
    return m


def test_extended_rows_and_one_tile_step():
    rng = np.random.default_rng(9)
    nt = [3, 2, 3]
    bits = rng.random((24, 16, 24)) < 0.3
    reached = _mask_of(bits, nt)
    pad = np.zeros((26, 18, 26), bool)
    pad[1:-1, 1:-1, 1:-1] = bits
    for t in itertools.product(range(3), range(2), range(3)):
        for conn in (6, 26):
            for e in range(100):
                ey, ez = e % 10, e // 10
                shell_y, shell_z = ey in (0, 9), ez in (0, 9)
                row = pad[t[2] * 8 + ez, t[1] * 8 + ey, t[0] * 8:t[0] * 8 + 10]
                exp = sum(int(b) << i for i, b in enumerate(row))
                if conn == 6 and shell_y and shell_z:
                    exp = 0
                elif conn == 6 and (shell_y or shell_z):
                    exp &= 0x1FE
                assert N.ext_row(conn, reached, nt, t, e) == exp, (t, conn, e)
    # one step: the component of the reached bits and the shell within the tile, by the reference
    for conn in (6, 26):
        for trial in range(20):
            passable = rng.random((8, 8, 8)) < (0.45 if conn == 6 else 0.2)
            ext = np.zeros((10, 10, 10), bool)
            ext[0, 1:9, 1:9] = rng.random((8, 8)) < 0.1                # a shell face
            ext[1:9, 1:9, 9] = rng.random((8, 8)) < 0.1
            if conn == 26:
                ext[9, 9, 9] = True; ext[0, 0, 1:9] = rng.random(8) < 0.3
            s = tuple(int(v) for v in rng.integers(0, 8, 3))
            ext[s[2] + 1, s[1] + 1, s[0] + 1] = passable[s[2], s[1], s[0]]
            rows = np.array([sum(int(b) << i for i, b in enumerate(ext[e // 10, e % 10])) for e in range(100)], np.uint32)
            pbytes = np.array([sum(int(b) << i for i, b in enumerate(passable[l >> 3, l & 7])) for l in range(64)], np.uint8)
            gained, after = N.tile_relax(conn, pbytes, rows)
            exp = _step_reference(passable, ext, conn)
            got = np.array([[(int(after[ez * 10 + ey]) >> i) & 1 for i in range(10)] for ez in range(10) for ey in range(10)], bool).reshape(10, 10, 10)
            assert (got == exp).all(), (conn, trial)
            assert gained == bool((got & ~ext).any())


def _step_reference(passable, ext, conn):
    """what one step computes: a search from every set bit of the 10^3 block that enters passable voxels of the tile only (the
    shell is a source, and does not change during a step)"""
    reach = ext.copy()
    frontier = [(int(x), int(y), int(z)) for z, y, x in zip(*np.nonzero(ext))]
    offs = F.offsets(conn)
    while frontier:
        nxt = []
        for x, y, z in frontier:
            for dx, dy, dz in offs:
                n = (x + dx, y + dy, z + dz)
                if all(1 <= v <= 8 for v in n) and passable[n[2] - 1, n[1] - 1, n[0] - 1] and not reach[n[2], n[1], n[0]]:
                    reach[n[2], n[1], n[0]] = True; nxt.append(n)
        frontier = nxt
    return reach


def test_wake_mask():
    def bit(dx, dy, dz):
        return 1 << ((dx + 1) + 3 * (dy + 1) + 9 * (dz + 1))
    assert N.wake_mask(6, 0x10, 0x10, 3, 3) == 0 and N.wake_mask(26, 0xFF, 0xFF, 0, 0) == 0          # nothing gained
    assert N.wake_mask(6, 0, 0x10, 3, 3) == 0 and N.wake_mask(26, 0, 0x7E, 3, 3) == 0                 # gained inside the tile
    for conn in (6, 26):
        for x, y, z in itertools.product((0, 3, 7), repeat=3):
            exp = 0
            for dx, dy, dz in F.offsets(conn):
                sees = all(d == 0 or v == (7 if d > 0 else 0) for d, v in zip((dx, dy, dz), (x, y, z)))
                exp |= bit(dx, dy, dz) if sees else 0
            assert N.wake_mask(conn, 0x00, 1 << x, y, z) == exp, (conn, x, y, z)
            assert N.wake_mask(conn, 1 << x, 1 << x | 0x10, y, z) == N.wake_mask(conn, 0, 0x10, y, z)   # only gained bits count


@pytest.mark.parametrize("conn,p", [(6, fc.P6), (26, fc.P26)])
def test_random_volumes_near_the_threshold(conn, p):
    for k, dims in enumerate(((33, 21, 19), (16, 16, 16), (41, 9, 26))):
        vol = fc.random_volume(dims, p, 100 * conn + k)
        rng = np.random.default_rng(k)
        solid = np.argwhere(vol != 0)
        empty = np.argwhere(vol == 0)
        for match in (F.SAME, F.SOLID):
            for pick in (solid, empty):
                z, y, x = (int(v) for v in pick[int(rng.integers(len(pick)))])
                same(vol, (x, y, z), 200, match, conn)
                # bounds whose lo and sizes are no multiple of 8, around the seed
                lo = (max(0, x - 5), max(0, y - 3), max(0, z - 7))
                same(vol, (x, y, z), 0, match, conn, (lo, (13, 11, 10)))
        # the largest solid cluster, so that the flood has somewhere to go
        sizes = [(F.region(vol, (int(x), int(y), int(z)), F.SOLID, conn)[0], (int(x), int(y), int(z))) for z, y, x in solid[::max(1, len(solid) // 12)]]
        n, s = max(sizes)
        assert n > 20
        _, res = same(vol, s, 201, F.SOLID, conn)
        assert res["region"] == n and res["changed"] == n


def test_the_small_scenes():
    vol, seed, n = fc.plus_volume()
    for conn in (6, 26):
        assert same(vol, seed, 9, F.SAME, conn)[1]["region"] == n
        assert same(vol, (4, 12, 12), 9, F.SOLID, conn)[1]["region"] == n
    for kind, a in itertools.product(("edge", "corner"), (8, 12)):
        vol, sa, sb = fc.diagonal_volume(kind, a)
        assert same(vol, sa, 9, F.SAME, 6)[1]["region"] == 8
        assert same(vol, sa, 9, F.SAME, 26)[1]["region"] == 16
        assert same(vol, sb, 9, F.SOLID, 26)[1]["region"] == 16
    vol, end, steps = fc.maze_volume(4)
    assert steps > 80
    assert same(vol, end, 3, F.SAME, 6)[1]["region"] == 127
    same(vol, end, 3, F.SAME, 26)
    vol, first, mid, path = fc.serpentine_volume()
    for conn in (6, 26):
        for s in (first, mid, path[-1]):
            assert same(vol, s, 2, F.SAME, conn)[1]["region"] == len(path)
    rounds = N.flood(vol, first, 2, F.SAME, 6, order="stale")[3]
    assert rounds >= 12 * 2 + 2 + 1        # a round per tile plane crossed (two in x on each of 12 rows, two in y), and the round that marks nothing
    cut = path[len(path) // 3]
    vol, first, mid, path = fc.serpentine_volume(cut=cut[:2])
    assert same(vol, first, 2, F.SAME, 6)[1]["region"] == len(path) // 3
    assert same(vol, mid, 2, F.SAME, 6)[1]["region"] == len(path) - len(path) // 3 - 1
    vol, inside, n = fc.cavity_volume()
    assert same(vol, inside, 5, F.SAME, 6, ((8, 4, 6), (20, 14, 16)))[1]["region"] == n + 1          # the hole itself, and no further
    assert same(vol, inside, 5, F.SAME, 6, ((-4, -4, -4), (34, 40, 40)))[1]["region"] == 30 * 24 * 32 - (20 * 14 * 16 - n - 1)    # bounds partly outside the volume: all the air of x < 30
    assert same(vol, inside, 5, F.SAME, 6, ((100, 0, 0), (4, 4, 4)))[1] == F.ZERO                      # bounds wholly outside
    assert same(vol, inside, 5, F.SAME, 6, ((0, 0, 0), (8, 8, 8)))[1] == F.ZERO                        # the seed outside the bounds
    assert same(vol, (0, 0, 0), 5, F.SOLID, 6)[1] == dict(F.ZERO)                                       # an empty seed under SOLID
    assert same(vol, inside, 0, F.SAME, 6)[1]["changed"] == 0                                           # the id already there


def test_clip_sides_and_loop_bound():
    vol = np.zeros((2, 3, 600), np.uint8)
    assert N.flood(vol, (0, 0, 0), 1, bounds=((0, 0, 0), (513, 3, 2)))[0] == 1
    assert N.flood(vol, (0, 0, 0), 1, bounds=((-50, 0, 0), (562, 3, 2)))[0] == 0                       # 512 after the clip
    assert N.flood(vol, (0, 0, 0), 1, bounds=((-50, 0, 0), (563, 3, 2)))[0] == 1
    rc, out, res, rounds = N.flood(vol, (88, 1, 1), 1, bounds=((88, 0, 0), (512, 3, 2)))
    assert rc == 0 and res["region"] == 512 * 6 and res["lo"] == (88, 0, 0) and res["size"] == (512, 3, 2) and (out[:, :, 88:] == 1).all() and not out[:, :, :88].any()
    # every round but the last gains a bit: the worst case, a line of single voxels flooded from one end tile by tile, stays far
    # below voxels + 1
    for order in ORDERS:
        rounds = N.flood(vol, (0, 0, 0), 1, bounds=((0, 0, 0), (512, 1, 1)), order=order)[3]
        assert 1 <= rounds <= N.round_bound((512, 1, 1))
    assert N.flood(vol, (511, 0, 0), 1, bounds=((0, 0, 0), (512, 1, 1)), order="stale")[3] == 64 + 1   # a tile a round, and the round that marks nothing


def test_fuzz_program_under_asan_and_ubsan(tmp_path):
    """tests/native/flood_fuzz.cpp, a program of its own, with -fsanitize=address,undefined and no recovery: the tiled algorithm in
    every tile order against a queue of voxels, with bounds and seeds at the int32 edges; an overflow or a mask index out of
    range would end it"""
    import os
    import re
    import subprocess
    src = os.path.join(N.ROOT, "tests", "native", "flood_fuzz.cpp")
    exe = str(tmp_path / "flood_fuzz_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, src])
    for seed in ("1", "2"):
        r = subprocess.run([exe, seed, "300"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
        m = re.match(r"(\d+) floods, (\d+) voxels reached", r.stdout)
        assert m and int(m.group(1)) == 1200 and int(m.group(2)) > 10_000, r.stdout
