"""What the GPU tests of vrt_scene_brush and vrt_scene_stamp share: the awkward scenes, the comparison of a scene's device
structures with a fresh build's (that of tests/test_gpu_scene_edit.py and tests/test_gpu_brick_edit.py, restated), the seeded
brush sequence, and the small frame held against the oracle."""
import numpy as np

import brush_reference as R

GB = ["color8", "depth", "motion", "mask8", "position", "normal8"]
DENSE_STATES = ("VOX", "DF", "OCC1", "OCC2", "OCC3")
BRICK_STATES = ("BENTRY", "BPOOL", "BFINE", "CELLS")
PTR = np.uint64(0xFFFFFF)
RES = (44, 28)
METAL_ID, ABSENT_ID, BLOCK_ID = 230, 199, 40                   # 200..255 are metallic in the tests' palette; 199 is in no volume

DENSE_A = (70, 45, 52)                                          # no side a multiple of 4, 8 or 64
DENSE_B = (150, 9, 11)                                          # a row is more than two segments of 64, and wider than the edits' cap of 127
BRICKS = (72, 48, 56)                                           # 9 x 6 x 7 bricks
BRICK_SPARE = 64                                                # free slots of the reserved brick scene


def dense_volume(dims, seed):
    W, H, D = dims
    rng = np.random.default_rng(seed)
    vol = ((rng.random((D, H, W)) < 0.02) * rng.integers(1, 199, (D, H, W))).astype(np.uint8)
    vol[D // 2:D // 2 + 4, H // 3:H // 3 + 3, W // 4:W // 4 + 30] = BLOCK_ID
    return vol


def brick_volume(dims, seed):
    """about a third of the bricks occupied, each sparsely"""
    W, H, D = dims
    rng = np.random.default_rng(seed)
    occ = rng.random((D // 8, H // 8, W // 8)) < 0.33
    vol = ((rng.random((D, H, W)) < 0.05) * rng.integers(1, 199, (D, H, W))).astype(np.uint8)
    vol *= np.repeat(np.repeat(np.repeat(occ, 8, 0), 8, 1), 8, 2).astype(np.uint8)
    vol[24:28, 16:19, 18:48] = BLOCK_ID
    return vol


def brick_occupancy(vol):
    D, H, W = vol.shape
    return vol.reshape(D // 8, 8, H // 8, 8, W // 8, 8).any(axis=(1, 3, 5))


def make_scene(vrt, engine, vol, pal, bricks, sky=None, noise=None, spare=BRICK_SPARE):
    if not bricks:
        return vrt.VoxelScene.from_dense(engine, vol, pal, sky=sky, noise=noise)
    grid, pool = vrt.synthetic.bricks_from_dense(vol)
    sc = vrt.VoxelScene.from_bricks(engine, grid, pool, pal, sky=sky, noise=noise)
    if spare is not None:
        sc.reserve_bricks(pool.shape[0] + spare)
    return sc


def snapshot(vrt, sc, bricks):
    return [sc.debug_state(getattr(vrt._capi, "STATE_" + n)).copy() for n in (BRICK_STATES if bricks else DENSE_STATES + ("CELLS",))]


def same_snapshot(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and (x == y).all() for x, y in zip(a, b))


def assert_state_equals_fresh(vrt, engine, sc, vol, pal, bricks, what):
    """every structure vrt_debug_scene_state knows equals that of a scene newly built from vol: byte for byte on a dense scene (the
    cell list as a sorted array), up to which pool slot a brick lies in on a brick scene"""
    K = vrt._capi
    fresh = make_scene(vrt, engine, vol, pal, bricks, spare=None)
    try:
        if not bricks:
            for n in DENSE_STATES:
                a, b = sc.debug_state(getattr(K, "STATE_" + n)), fresh.debug_state(getattr(K, "STATE_" + n))
                assert a.shape == b.shape, (what, n, a.shape, b.shape)
                if not (a == b).all():
                    i = np.flatnonzero(a != b)
                    raise AssertionError(f"{what}: {n} differs in {i.size} places, first at {int(i[0])}: {int(a.flat[i[0]])} != {int(b.flat[i[0]])}")
            ca, cb = np.sort(sc.debug_state(K.STATE_CELLS)), np.sort(fresh.debug_state(K.STATE_CELLS))
            assert ca.shape == cb.shape and (ca == cb).all(), (what, "CELLS")
            return
        ea, pa, fa = (sc.debug_state(getattr(K, "STATE_" + n)) for n in BRICK_STATES[:3])
        eb, pb, fb = (fresh.debug_state(getattr(K, "STATE_" + n)) for n in BRICK_STATES[:3])
        ca, cb = np.sort(sc.debug_state(K.STATE_CELLS)), np.sort(fresh.debug_state(K.STATE_CELLS))
        assert ea.shape == eb.shape, (what, ea.shape, eb.shape)
        diff = np.flatnonzero((ea & ~PTR) != (eb & ~PTR))
        assert diff.size == 0, f"{what}: {diff.size} entries differ beside the pointer, first at padded index {int(diff[0])}"
        ptr_a, ptr_b = (ea & PTR).astype(np.int64), (eb & PTR).astype(np.int64)
        kind = lambda p: np.where(p == 0, 0, np.where(p == 0xFFFFFF, 2, 1))               # empty / occupied / border
        assert (kind(ptr_a) == kind(ptr_b)).all(), (what, "pointers")
        occ = kind(ptr_a) == 1
        n_occ = int(occ.sum())
        assert n_occ == pb.shape[0] and len(set(ptr_a[occ].tolist())) == n_occ, (what, "slots")
        assert int(ptr_a[occ].max(initial=0)) <= pa.shape[0], (what, "a pointer past the pool")
        assert (pa[ptr_a[occ] - 1] == pb[ptr_b[occ] - 1]).all(), (what, "ids")
        bad = np.flatnonzero((fa[ptr_a[occ] - 1] != fb[ptr_b[occ] - 1]).reshape(n_occ, 8 * 512).any(axis=1))
        assert bad.size == 0, f"{what}: the fine bytes of {bad.size} bricks differ"
        assert ca.shape == cb.shape and (ca == cb).all(), (what, "cells")
    finally:
        fresh.destroy()


def whole(sc, dims):
    return sc.read((0, 0, 0), dims)


# ---- the brush sequence ---------------------------------------------------------------------------------------------------------
def op(kind, shape, mode, p, vid=0, match=0):
    return {"kind": kind, "shape": shape, "mode": mode, "p": [int(v) for v in p], "id": vid, "match": match}


def sphere(c, r):
    """centre in voxels (multiples of 0.5), radius in voxels -> an ellipsoid's parameters"""
    return [int(round(2 * v)) for v in c] + [int(round(2 * r))] * 3


def brush_sequence(dims, seed):
    """at least 40 brushes; every one is legal, what it does is the reference's business.  Kinds that must be a no-op are marked
    'no-op: ...'; the one that must be refused on the brick scene 'needs more slots'."""
    W, H, D = dims
    rng = np.random.default_rng(seed)

    def at(m=3):                                                 # a voxel at least m from every face, where the volume is that thick
        lo = [min(m, (dims[a] - 1) // 2) for a in range(3)]
        return [int(rng.integers(lo[a], max(lo[a] + 1, dims[a] - m))) for a in range(3)]
    seq = []
    # every shape times every mode
    for mode, vid, match in ((R.SET, 21, 0), (R.PAINT, 22, 0), (R.ADD, 23, 0), (R.REPLACE, 24, BLOCK_ID)):
        c = at()
        seq.append(op("box x mode %d" % mode, R.BOX, mode, [c[0] - 4, c[1] - 2, c[2] - 3, 9, 5, 7], vid, match))
        c = at()
        seq.append(op("ellipsoid x mode %d" % mode, R.ELLIPSOID, mode, [2 * c[0] + 1, 2 * c[1], 2 * c[2] + 1, 11, 6, 8], vid + 4, match))
        c, e = at(), at()
        seq.append(op("capsule x mode %d" % mode, R.CAPSULE, mode, [2 * c[0], 2 * c[1] + 1, 2 * c[2], 2 * e[0] + 1, 2 * e[1], 2 * e[2], 5], vid + 8, match))
    seq.append(op("replace the block", R.BOX, R.REPLACE, [0, 0, 0, W, H, D], 41, BLOCK_ID))
    # bricks: a carve that empties whole bricks, an ADD that makes bricks appear (the ADD that needs more slots than are free: below)
    seq.append(op("carve that empties bricks", R.BOX, R.SET, [6, 5, 3, 29, 22, 27], 0))
    seq.append(op("add that makes bricks appear", R.ELLIPSOID, R.ADD, sphere((20.5, 16.0, 16.5), 9.5), 70))
    # clipped by each face and by a corner; wholly outside
    for a in range(3):
        for far in (0, 1):
            c = [dims[b] / 2.0 for b in range(3)]
            c[a] = float(dims[a]) if far else 0.0
            seq.append(op("clipped by face %d%s" % (a, "+" if far else "-"), R.ELLIPSOID, R.SET, sphere(c, 3.5), 50 + 2 * a + far))
    seq.append(op("clipped by a corner", R.ELLIPSOID, R.SET, sphere((W, H, D), 4.0), 57))
    seq.append(op("clipped by the other corner", R.CAPSULE, R.SET, [-9, -7, -8, 5, 6, 3, 6], 58))
    seq.append(op("no-op: wholly outside", R.ELLIPSOID, R.SET, sphere((-20, H / 2.0, D / 2.0), 6.0), 59))
    seq.append(op("no-op: a box beyond the far corner", R.BOX, R.SET, [W, H, D, 5, 5, 5], 59))
    # the no-ops: SET of the id already there, PAINT over air, REPLACE of an absent id
    c = at(5)
    room = [c[0] - 3, c[1] - 3, c[2] - 3, 7, 7, 7]
    seq.append(op("carve a room", R.BOX, R.SET, room, 0))
    seq.append(op("no-op: paint over air", R.ELLIPSOID, R.PAINT, sphere([v + 0.5 for v in c], 2.5), 60))
    seq.append(op("no-op: carve the room again", R.BOX, R.SET, room, 0))
    seq.append(op("fill the room", R.BOX, R.SET, room, 61))
    seq.append(op("no-op: set the id already there", R.ELLIPSOID, R.SET, sphere([v + 0.5 for v in c], 2.5), 61))
    seq.append(op("no-op: add into the full room", R.BOX, R.ADD, room, 62))
    seq.append(op("no-op: replace an absent id", R.BOX, R.REPLACE, [0, 0, 0, W, H, D], 63, ABSENT_ID))
    # one voxel; a degenerate capsule
    c = at()
    seq.append(op("one-voxel ellipsoid", R.ELLIPSOID, R.SET, [2 * c[0] + 1, 2 * c[1] + 1, 2 * c[2] + 1, 1, 1, 1], 64))
    seq.append(op("one-voxel ellipsoid, carved", R.ELLIPSOID, R.SET, [2 * c[0] + 1, 2 * c[1] + 1, 2 * c[2] + 1, 1, 1, 1], 0))
    c = at()
    seq.append(op("degenerate capsule", R.CAPSULE, R.SET, [2 * c[0], 2 * c[1], 2 * c[2]] * 2 + [5], 65))
    # bounds that start at an odd x and span one, two and three segments (as far as the volume is wide)
    for k, n in enumerate((30, 100, 140)):
        n = min(n, W - 5)
        seq.append(op("odd x, %d wide" % n, R.BOX, R.PAINT if k == 1 else R.SET, [5, 1 + k, 2 + k, n, 2, 2], 66 + k))
    seq.append(op("a capsule along x", R.CAPSULE, R.ADD, [7, H, D, 2 * W - 9, H + 1, D - 1, 3], 69))
    seq.append(op("needs more slots", R.BOX, R.ADD, [0, 0, 0, W, H, D], 71))
    seq.append(op("carve a sphere out of it", R.ELLIPSOID, R.SET, sphere((W / 2.0, H / 2.0, D / 2.0), min(H, D) / 2.0 - 1), 0))
    # metal into a scene that has none
    c = at()
    seq.append(op("metallic id", R.ELLIPSOID, R.SET, sphere((W / 2.0, H / 2.0, 3.0), 3.5), METAL_ID))
    seq.append(op("paint it over", R.BOX, R.PAINT, [0, 0, 0, W, H, 8], 72))
    return seq


def needs_more_slots(vol, out, free_slots):
    """the brick edits' own rule, for whichever tool rewrote vol into out, from the numpy volumes: the bricks that appear are more
    than the free slots and the slots of the bricks that vanish"""
    before, after = brick_occupancy(vol), brick_occupancy(out)
    appear, vanish = int((after & ~before).sum()), int((before & ~after).sum())
    return appear > free_slots + vanish


def expected(vol, o, bricks, free_slots):
    """-> (the volume after, (changed, lo, size), refused): refused is the brick edits' own rule, from the numpy volumes"""
    out, res = R.brush(vol, o["shape"], o["mode"], o["p"], o["id"], o["match"])
    if bricks and res[0] and needs_more_slots(vol, out, free_slots):
        return vol, (0, [0, 0, 0], [0, 0, 0]), True
    return out, res, False


# ---- the small frame --------------------------------------------------------------------------------------------------------------
def frame_setup(vrt, dims):
    W, H, D = dims
    st = vrt.VoxelRenderSettings(targetResolution=RES)           # the reference's defaults: AO 4, shadows, 5 bounces
    st.fsrSetttings.enable = False
    cam = vrt.CameraController(position=(W / 2 + 0.3, H / 2 + 0.2, -0.9 * max(W, D)))
    return st, vrt.make_push(cam, dims, RES, frame=2)


def assert_frame_equals_oracle(vrt, oracle, engine, sc, vol, pal, sky, noise, dims, what, planes=GB):
    from helpers import compare_planes
    st, push = frame_setup(vrt, dims)
    gb = vrt.GeometryStage(engine, st, sc, debug_planes=planes is not GB).record(push)
    engine.synchronize()
    exp = oracle.render(oracle.OracleScene(vol, pal, sky=sky, noise=noise), push, oracle.params_from(st.to_c()), planes=planes, nthreads=8)
    bad = compare_planes(gb.numpy(), exp, planes)
    assert not bad, (what, bad)
    return exp
