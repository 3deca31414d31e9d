"""What vrt_scene_from_dense and vrt_scene_from_bricks build on the device -- the eight octant clearance fields with their open
cells, the padded voxel ids, the occupancy pyramid, the occupied-cell list; of brick scenes the packed entries, the pool and the
per-voxel clearances -- against the definitions of tests/scene_reference.py (numpy, from the volume alone; held against brute
force in tests/test_scene_reference_cpu.py).  Every comparison is exact equality of everything vrt_debug_scene_state hands out:
sizes first, then every byte, borders, rounding tails and sentinel included.  The edit tests (test_gpu_scene_edit.py,
test_gpu_brick_edit.py) compare an edited scene with a fresh build; this file says what a fresh build is."""
import functools
import time

import numpy as np
import pytest

import extents_common
import scene_reference as R
from helpers import metallic_palette
from test_gpu_scene_edit import apply_edit

pytestmark = pytest.mark.gpu

TOTAL = {"cases": 0, "bytes": 0}


def count(case_bytes):
    TOTAL["cases"] += 1
    TOTAL["bytes"] += int(case_bytes)


# ---- dense scenes -----------------------------------------------------------------------------------------------------------------

DIMS = [(1, 1, 1), (1, 1, 200), (200, 1, 1), (3, 5, 7), (4, 4, 4), (5, 4, 4), (63, 9, 10), (64, 8, 8), (65, 8, 8), (255, 3, 5), (256, 4, 4),
        (257, 6, 3), (300, 40, 20), (17, 70, 66), (130, 129, 131)]
# the longest axis a scene may have (tests/extents_common.py): cells 0 .. 1023 of the cell list, rows of 4098 bytes
NEEDLES = extents_common.NEEDLES + extents_common.RAGGED
DIMS += NEEDLES + extents_common.LINES
CORNERS = [(3, 5, 7), (5, 4, 4), (65, 8, 8), (257, 6, 3), (17, 70, 66), (130, 129, 131)] + NEEDLES
DENSITIES = [(1, 1, 200), (200, 1, 1), (63, 9, 10), (64, 8, 8), (255, 3, 5), (256, 4, 4), (300, 40, 20), (17, 70, 66), (130, 129, 131)] + NEEDLES
SLABS = [(3, 5, 7), (63, 9, 10), (65, 8, 8), (257, 6, 3), (300, 40, 20), (130, 129, 131)]


def dense_contents(dims):
    """[(name, vol[z, y, x])] for one W x H x D"""
    W, H, D = dims
    rng = np.random.default_rng(W * 1000003 + H * 1009 + D)
    rand = lambda p: ((rng.random((D, H, W)) < p) * rng.integers(1, 256, (D, H, W))).astype(np.uint8)
    out = [("empty", np.zeros((D, H, W), np.uint8)), ("full", rng.integers(1, 256, (D, H, W)).astype(np.uint8))]
    v = np.zeros((D, H, W), np.uint8); v[D // 2, H // 2, W // 2] = 200
    out += [("one voxel in the centre", v), ("random 0.05", rand(0.05))]
    if dims in CORNERS:
        for k in range(8):
            v = np.zeros((D, H, W), np.uint8)
            v[(D - 1) * (k >> 2), (H - 1) * (k >> 1 & 1), (W - 1) * (k & 1)] = 1 + k
            out.append((f"one voxel in corner {k}", v))
    if dims in DENSITIES:
        out += [("random 0.002", rand(0.002)), ("random 0.5", rand(0.5))]
    if dims in NEEDLES:
        out.append(("the needle of extents_common", extents_common.needle_volume(dims)))
    if dims in SLABS:
        for axis, name in ((2, "x"), (1, "y"), (0, "z")):
            v = np.zeros((D, H, W), np.uint8)
            idx = [slice(None)] * 3
            idx[axis] = (D, H, W)[axis] // 2
            v[tuple(idx)] = 9
            out.append((f"a slab across {name}", v))
    return out


@functools.lru_cache(maxsize=None)
def dense_case_list():
    import voxel_raytracing_amd as vrt
    cases = [(dims, name, vol) for dims in DIMS for name, vol in dense_contents(dims)]
    cases.append(((48, 48, 48), "treehouse", vrt.synthetic.treehouse(48)))
    return cases


_REFERENCE = {}


def dense_reference(dims, name, vol):
    """(clearances [8, z, y, x], open cells [8, z, y, x]) of a case, computed once"""
    key = (dims, name)
    if key not in _REFERENCE:
        _REFERENCE[key] = (R.dense_fields(vol, False), np.stack([R.open_cells(vol, o) for o in range(8)]))
    return _REFERENCE[key]


def check_dense_scene(vrt, sc, vol, fields, what):
    K = vrt._capi
    D, H, W = vol.shape
    dims = (W, H, D)
    got = sc.debug_state(K.STATE_VOX)
    assert got.shape == (vol.size,) and (got == vol.reshape(-1)).all(), (what, "VOX")
    df = sc.debug_state(K.STATE_DF)
    assert df.size == 9 * R.df_field_bytes(W, H, D) + 256, (what, "DF size", df.size)
    msg = R.diff_df(df, R.dense_df_bytes(vol, None, fields), dims, what)
    assert msg is None, msg
    n = got.nbytes + df.nbytes
    for k, (name, ref) in enumerate(zip(("OCC1", "OCC2", "OCC3"), R.pyramid(vol))):
        lv = sc.debug_state(getattr(K, "STATE_" + name))
        msg = R.diff_words(lv, ref, name, R.level_dims(dims, k + 1), what)
        assert msg is None, msg
        n += lv.nbytes
    cl = sc.debug_state(K.STATE_CELLS)
    msg = R.diff_cells(cl, R.cells(vol), what)
    assert msg is None, msg
    count(n + cl.nbytes)


def run_dense_case(vrt, engine, dims, name, vol):
    clear, op = dense_reference(dims, name, vol)
    opened = np.where(op, np.uint8(0), clear)
    pal = metallic_palette(vrt)
    with engine.options(open_cells=0):
        sc = vrt.VoxelScene.from_dense(engine, vol, pal)
    try:
        check_dense_scene(vrt, sc, vol, clear, f"{dims} {name}, open_cells=0")
    finally:
        sc.destroy()
    sc = vrt.VoxelScene.from_dense(engine, vol, pal)
    try:
        check_dense_scene(vrt, sc, vol, opened, f"{dims} {name}")
    finally:
        sc.destroy()


@pytest.mark.parametrize("dims", DIMS + [(48, 48, 48)], ids=lambda d: "x".join(str(v) for v in d))
def test_dense_build_equals_the_definition(vrt, engine, dims):
    t0 = time.time()
    mine = [c for c in dense_case_list() if c[0] == dims]
    assert mine
    for _, name, vol in mine:
        assert vol.shape == dims[::-1]
        run_dense_case(vrt, engine, dims, name, vol)
    print(f"{dims}: {len(mine)} volumes x 2 builds in {time.time() - t0:.1f} s; so far {TOTAL['cases']} scenes, {TOTAL['bytes']} bytes compared")


def test_the_dense_cases_exercise_the_classes():
    """over the set: a field reaches the cap; values in 64..126 occur; some row has open cells in more than one 64-lane chunk of
    k_open_x, and some row a chunk with a blocked cell between a chunk with open cells and one whose cells would be open but for
    the carry; open and non-open empty cells occur in every octant"""
    reaches_cap = mid_values = two_chunks = blocked_between = False
    open_seen, closed_seen = set(), set()
    for dims, name, vol in dense_case_list():
        clear, op = dense_reference(dims, name, vol)
        reaches_cap |= bool((clear == R.DF_CAP).any())
        mid_values |= bool(((clear >= 64) & (clear < R.DF_CAP)).any())
        W = dims[0]
        for o in range(8):
            if op[o].any():
                open_seen.add(o)
            if ((vol == 0) & ~op[o]).any():
                closed_seen.add(o)
            if W <= 64 or (two_chunks and blocked_between):
                continue
            sx = R.signs(o)[0]
            # what k_open_x reads: the cell and everything beyond it along y and z is empty (x still to be scanned)
            f = R._flip_to_positive(vol == 0, o)
            for axis in (0, 1):
                f = np.flip(np.logical_and.accumulate(np.flip(f, axis), axis), axis)
            f = R._flip_to_positive(f, o).reshape(-1, W)
            rows_open = op[o].reshape(-1, W)
            nchunk = (W + 63) // 64
            pad = nchunk * 64 - W
            chunked = lambda a, fill: np.concatenate([a, np.full((a.shape[0], pad), fill)], axis=1).reshape(-1, nchunk, 64)
            any_open, any_blocked, any_flag = chunked(rows_open, False).any(2), (~chunked(f, True)).any(2), chunked(f & ~rows_open, False).any(2)
            if sx > 0:                                            # the scan starts at the far end of the row
                any_open, any_blocked, any_flag = any_open[:, ::-1], any_blocked[:, ::-1], any_flag[:, ::-1]
            two_chunks |= bool((any_open.sum(1) > 1).any())
            for r in np.flatnonzero(any_open.any(1) & any_blocked.any(1)):
                a, b = int(np.argmax(any_open[r])), np.flatnonzero(any_blocked[r])
                b = b[b > a]
                if b.size and any_flag[r, int(b[0]) + 1:].any():
                    blocked_between = True
                    break
    assert reaches_cap and mid_values and two_chunks and blocked_between, (reaches_cap, mid_values, two_chunks, blocked_between)
    assert open_seen == set(range(8)) and closed_seen == set(range(8)), (open_seen, closed_seen)


# ---- brick scenes -----------------------------------------------------------------------------------------------------------------

GRIDS = [(1, 1, 1), (1, 1, 20), (20, 1, 1), (3, 4, 5), (12, 8, 11), (17, 16, 18)]          # bricks: nbx, nby, nbz
GRIDS += extents_common.BRICK_NEEDLES                             # the longest axis, 512 bricks: brick coordinates 0 .. 511


def sparse_brick(rng, p=0.05):
    b = ((rng.random((8, 8, 8)) < p) * rng.integers(1, 256, (8, 8, 8))).astype(np.uint8)
    b[int(rng.integers(0, 8)), int(rng.integers(0, 8)), int(rng.integers(0, 8))] = 3
    return b


def brick_contents(nb):
    nbx, nby, nbz = nb
    W, H, D = nbx * 8, nby * 8, nbz * 8
    rng = np.random.default_rng(nbx * 10007 + nby * 101 + nbz)
    put = lambda v, b, ids: v.__setitem__((slice(b[2] * 8, b[2] * 8 + 8), slice(b[1] * 8, b[1] * 8 + 8), slice(b[0] * 8, b[0] * 8 + 8)), ids)
    out = [("empty", np.zeros((D, H, W), np.uint8))]
    v = np.zeros((D, H, W), np.uint8); put(v, (nbx - 1, 0, nbz - 1), sparse_brick(rng))
    out.append(("one brick at a corner", v))
    v = np.zeros((D, H, W), np.uint8); put(v, (nbx // 2, nby // 2, nbz // 2), sparse_brick(rng))
    out.append(("one brick in the middle", v))
    if nb == (17, 16, 18):
        return out
    # sparse voxels, some full bricks beside sparse ones, voxels on every wall
    v = ((rng.random((D, H, W)) < 0.0015) * rng.integers(1, 256, (D, H, W))).astype(np.uint8)
    for _ in range(max(1, nbx * nby * nbz // 12)):
        b = [int(rng.integers(0, n)) for n in nb]
        put(v, b, rng.integers(1, 256, (8, 8, 8)).astype(np.uint8))
        nbr = [min(b[0] + 1, nbx - 1), b[1], b[2]]
        if nbr != b:
            put(v, nbr, sparse_brick(rng))
    for x, y, z in ((0, H // 2, D // 2), (W - 1, H // 3, D // 3), (W // 2, 0, D // 2), (W // 3, H - 1, D // 3), (W // 2, H // 2, 0), (W // 3, H // 3, D - 1)):
        v[z, y, x] = 77
    out.append(("random sparse", v))
    # bricks whose only solid voxel sits in one of their eight corners, every second brick along each axis
    v = np.zeros((D, H, W), np.uint8)
    k = 0
    for bz in range(0, nbz, 2):
        for by in range(0, nby, 2):
            for bx in range(0, nbx, 2):
                v[bz * 8 + 7 * (k >> 2 & 1), by * 8 + 7 * (k >> 1 & 1), bx * 8 + 7 * (k & 1)] = 1 + k % 255
                k += 1
    out.append(("one corner voxel per brick", v))
    if nb in extents_common.BRICK_NEEDLES:
        out.append(("the needle of extents_common", extents_common.brick_needle_volume(nb)))
    if nb == (1, 1, 1):
        for k in range(1, 8):
            v = np.zeros((D, H, W), np.uint8)
            v[7 * (k >> 2 & 1), 7 * (k >> 1 & 1), 7 * (k & 1)] = 5
            out.append((f"the voxel in corner {k}", v))
    return out


def check_brick_scene(vrt, sc, vol, grid, open, slots, what):
    """grid: the pointers the scene was built from (a fresh build keeps them), or None with slots = the pool's size: occupied,
    distinct, inside the pool"""
    K = vrt._capi
    D, H, W = vol.shape
    nb = (W // 8, H // 8, D // 8)
    ent, pool, fine, cl = sc.debug_state(K.STATE_BENTRY), sc.debug_state(K.STATE_BPOOL), sc.debug_state(K.STATE_BFINE), sc.debug_state(K.STATE_CELLS)
    occ = R.brick_occupancy(vol)
    expect = R.brick_entries(occ if grid is None else grid, open)
    msg = R.diff_entries(ent, expect, nb, None if grid is not None else slots, what)
    assert msg is None, msg
    n_slots = int(occ.sum()) if slots is None else slots
    assert pool.shape == (n_slots, 512) and fine.shape == (n_slots, 8, 512), (what, pool.shape, fine.shape)
    msg = R.diff_brick_bytes(ent, pool, fine, vol, nb, what)
    assert msg is None, msg
    msg = R.diff_cells(cl, R.brick_cells(vol), what)
    assert msg is None, msg
    count(ent.nbytes + int(occ.sum()) * 512 * 9 + cl.nbytes)


@pytest.mark.parametrize("nb", GRIDS, ids=lambda d: "x".join(str(v) for v in d))
def test_brick_build_equals_the_definition(vrt, engine, nb):
    pal = metallic_palette(vrt)
    rng = np.random.default_rng(17)
    for name, vol in brick_contents(nb):
        what = f"{nb} bricks, {name}"
        grid, pool = vrt.synthetic.bricks_from_dense(vol)
        n = pool.shape[0]
        sc = vrt.VoxelScene.from_bricks(engine, grid, pool, pal)
        check_brick_scene(vrt, sc, vol, grid, True, None, what)
        sc.destroy()
        # the pool handed over in another slot order
        perm = rng.permutation(n)                                 # new slot j holds the old brick perm[j]
        inv = np.empty(n, np.int64); inv[perm] = np.arange(n)
        grid_p = np.where(grid != 0, inv[np.maximum(grid.astype(np.int64), 1) - 1] + 1, 0).astype(np.uint32) if n else grid
        sc = vrt.VoxelScene.from_bricks(engine, grid_p, pool[perm], pal)
        check_brick_scene(vrt, sc, vol, grid_p, True, None, what + ", permuted pool")
        sc.destroy()
        # without open bricks: the open bits are zero, all else as before
        with engine.options(open_cells=0):
            sc = vrt.VoxelScene.from_bricks(engine, grid, pool, pal)
        check_brick_scene(vrt, sc, vol, grid, False, None, what + ", open_cells=0")
        sc.destroy()
        # reserved: the coarse fields come back out of the entries (k_brick_unpack) and are built again
        sc = vrt.VoxelScene.from_bricks(engine, grid, pool, pal)
        sc.reserve_bricks(n + 5)
        check_brick_scene(vrt, sc, vol, None, True, n + 5, what + ", reserved")
        sc.destroy()


def test_the_brick_cases_exercise_the_classes():
    """a coarse clearance of 16 (stored as 15) needs 16 empty bricks along ALL three axes -- the clearance is a cube's side, so the
    1 x 1 x 20 grids stay at 1 and the 17 x 16 x 18 grid is what reaches it; per-voxel clearances of 9..15 look into the
    neighbouring bricks; open and non-open empty bricks occur in every octant"""
    coarse, fine_values = set(), set()
    open_seen, closed_seen = set(), set()
    for nb in GRIDS:
        for name, vol in brick_contents(nb):
            occ = R.brick_occupancy(vol).astype(np.uint8)
            for o in range(8):
                coarse.update(np.unique(R.clearance(occ, o, R.BRICK_CAP)).tolist())
                if nb[0] * nb[1] * nb[2] <= 1056 and occ.any():
                    fine_values.update(np.unique(R.to_bricks(R.brick_fine(vol, o))[occ != 0]).tolist())
                op = R.open_cells(occ, o)
                if op.any():
                    open_seen.add(o)
                if ((occ == 0) & ~op).any():
                    closed_seen.add(o)
    assert {0, 1, 2, 8, 15, 16} <= coarse, sorted(coarse)
    assert set(range(0, 16)) <= fine_values, sorted(fine_values)
    assert open_seen == set(range(8)) and closed_seen == set(range(8))


def test_edits_of_a_reserved_brick_scene_equal_the_definition(vrt, engine):
    """two edits, one that changes which bricks are occupied and one that does not, against the definition of the numpy-edited
    volume -- not against another build: the edit tests' "as a fresh build" then rests on this file's ground"""
    pal = metallic_palette(vrt)
    vol = dict(brick_contents((12, 8, 11)))["random sparse"].copy()
    grid, pool = vrt.synthetic.bricks_from_dense(vol)
    slots = pool.shape[0] + 40
    sc = vrt.VoxelScene.from_bricks(engine, grid, pool, pal)
    sc.reserve_bricks(slots)
    before = R.brick_occupancy(vol)
    empty = np.argwhere(~before[1:-1, 1:-1, 1:-2] & ~before[1:-1, 1:-1, 2:-1])[0] + 1     # two empty bricks side by side
    lo = [int(empty[2]) * 8 + 5, int(empty[1]) * 8 + 2, int(empty[0]) * 8 + 3]
    apply_edit(sc, vol, lo, ([7, 4, 3], 99))                      # straddles both
    assert int((R.brick_occupancy(vol) != before).sum()) == 2
    check_brick_scene(vrt, sc, vol, None, True, slots, "an edit that occupies two bricks")
    before = R.brick_occupancy(vol)
    z, y, x = (int(v) for v in np.argwhere(vol == 99)[0])
    rng = np.random.default_rng(2)
    ids = rng.integers(0, 3, (3, 3, 3)).astype(np.uint8) * 50
    ids[0, 0, 0] = 98
    apply_edit(sc, vol, [x, y, z], ids)                           # other ids and holes inside what the first edit wrote
    assert (R.brick_occupancy(vol) == before).all() and (ids == 0).any()
    check_brick_scene(vrt, sc, vol, None, True, slots, "an edit inside occupied bricks")
    sc.destroy()


# ---- the 64-bit field layout ------------------------------------------------------------------------------------------------------

def test_fields_of_a_volume_past_the_32bit_limit(vrt, engine):
    """the 832^3 scene of tests/test_gpu_configs.py: eight fields of 834^3 bytes, no field 8, every index 64 bits.  2000 points x 8
    octants against the point-wise reference (clearance by binary search over the cube's side, open cells by the box to the
    corner), the zero border of every field on a face per axis."""
    t0 = time.time()
    N = 832
    vol = vrt.synthetic.sparse_bricks(N, 8, 0.004, seed=9)
    sc = vrt.VoxelScene.from_dense(engine, vol, metallic_palette(vrt))
    df = sc.debug_state(vrt._capi.STATE_DF)
    sc.destroy()
    t1 = time.time()
    P = N + 2
    ndf = R.df_field_bytes(N, N, N)
    assert df.size == 8 * ndf and 8 * ndf > 1 << 32
    for o in range(8):
        f = df[o * ndf:o * ndf + P ** 3].reshape(P, P, P)
        assert not f[0].any() and not f[-1].any() and not f[:, 0].any() and not f[:, :, -1].any(), ("border of field", o)
        assert not df[o * ndf + P ** 3:(o + 1) * ndf].any(), ("rounding tail of field", o)
    t2 = time.time()
    ref = R.PointReference(vol)
    t3 = time.time()
    rng = np.random.default_rng(832)
    pts = [((N - 1) * (k & 1), (N - 1) * (k >> 1 & 1), (N - 1) * (k >> 2)) for k in range(8)]                      # the corners
    for a in range(3):                                            # on every face
        for side in (0, N - 1):
            for _ in range(20):
                p = [int(v) for v in rng.integers(0, N, 3)]
                p[a] = side
                pts.append(tuple(p))
    first = -(-((1 << 32) - 7 * ndf) // (P * P))                   # from this padded z on, field 7 lies past byte 2^32
    assert 0 < first < N
    pts += [(int(rng.integers(0, N)), int(rng.integers(0, N)), int(rng.integers(first, N))) for _ in range(300)]
    bz, by, bx = np.nonzero(vol[::8, ::8, ::8])                   # in and next to solid bricks
    for k in rng.choice(bx.size, 100, replace=False):
        x, y, z = int(bx[k]) * 8, int(by[k]) * 8, int(bz[k]) * 8
        pts += [(x + int(rng.integers(0, 8)), y + int(rng.integers(0, 8)), z + int(rng.integers(0, 8))), (max(x - 1, 0), y, z), (x, min(y + 8, N - 1), z)]
    pts += [tuple(int(v) for v in rng.integers(0, N, 3)) for _ in range(2000 - len(pts) + 400)]
    pts = list(dict.fromkeys(pts))
    assert len(pts) >= 2000
    kinds = {"solid": 0, "open": 0, "closed": 0, "64 and more": 0, "past 2^32": 0}
    for x, y, z in pts:
        for o in range(8):
            i = o * ndf + (x + 1) + ((y + 1) + (z + 1) * P) * P
            c = ref.clearance((x, y, z), o, R.DF_CAP)
            is_open = ref.open((x, y, z), o)
            kinds["solid"] += c == 0
            kinds["open"] += is_open
            kinds["closed"] += c > 0 and not is_open
            kinds["64 and more"] += c >= 64 and not is_open
            kinds["past 2^32"] += i >= 1 << 32
            assert int(df[i]) == (0 if is_open else c), f"field {o} x {x} y {y} z {z} (byte {i}): {int(df[i])} != {0 if is_open else c} (clearance {c}, open {is_open})"
    assert min(kinds.values()) >= 50, kinds
    count(8 * len(pts) + 8 * (4 * P * P + ndf - P ** 3))
    print(f"832^3: {len(pts)} points x 8 octants, {kinds}; build and download {t1 - t0:.1f} s, borders {t2 - t1:.1f} s, "
          f"summed-area table {t3 - t2:.1f} s, points {time.time() - t3:.1f} s, all {time.time() - t0:.1f} s")
