"""vrt_scene_flood on the GPU, held bit for bit to a plain breadth-first search (tests/flood_reference.py): single-purpose scenes
(a region inside one tile, through each face of a tile, diagonal contact on and off a tile edge, a maze inside one tile, a
serpentine that re-enters tiles, a leaking cavity), seeded floods on thinned volumes, and the API's rules (no-op, MEASURE,
bricks and their slots, metal, side limits, streams).  After every flood that changes something the scene's device structures
equal a fresh build's; one small frame per scene is held against the oracle."""
import ctypes as C
import itertools

import numpy as np
import pytest

import brush_common as bc
import flood_common as fc
import flood_reference as F
import stream_common as sc_
from helpers import metallic_palette

pytestmark = pytest.mark.gpu

BOTH = pytest.mark.parametrize("bricks", [False, True], ids=["dense", "bricks"])


def textures(vrt):
    return vrt.synthetic.sky_gradient(64, 32), vrt.synthetic.blue_noise_standin(64)


def dims_of(vol):
    return (vol.shape[2], vol.shape[1], vol.shape[0])


def flood(vrt, engine, sc, vol, pal, bricks, seed, vid, match, conn, bounds=None, what=""):
    """one flood on the scene and on the reference -> (the volume after, the result)"""
    exp_vol, exp = F.flood(vol, seed, vid, match, conn, bounds)
    before = bc.snapshot(vrt, sc, bricks) if exp["changed"] == 0 else None
    got = sc.flood(seed, vid, match, conn, bounds)
    print(what, seed, vid, match, conn, bounds, got, "rounds", sc.flood_rounds())
    assert got == exp, (what, got, exp)
    assert (bc.whole(sc, dims_of(vol)) == exp_vol).all(), what
    if exp["changed"]:
        bc.assert_state_equals_fresh(vrt, engine, sc, exp_vol, pal, bricks, what)
    else:
        assert bc.same_snapshot(before, bc.snapshot(vrt, sc, bricks)), what
    return exp_vol, exp


class Scene:
    """a scene of `vol` with textures, and the small frame against the oracle when it goes"""
    def __init__(self, vrt, oracle, engine, vol, bricks, spare=bc.BRICK_SPARE):
        self.vrt, self.oracle, self.engine, self.vol, self.bricks = vrt, oracle, engine, vol, bricks
        self.pal = metallic_palette(vrt)
        self.sky, self.noise = textures(vrt)
        self.sc = bc.make_scene(vrt, engine, vol, self.pal, bricks, sky=self.sky, noise=self.noise, spare=spare)

    def flood(self, seed, vid, match=F.SAME, conn=6, bounds=None, what=""):
        self.vol, res = flood(self.vrt, self.engine, self.sc, self.vol, self.pal, self.bricks, seed, vid, match, conn, bounds, what)
        return res

    def frame(self, what, planes=bc.GB):
        return bc.assert_frame_equals_oracle(self.vrt, self.oracle, self.engine, self.sc, self.vol, self.pal, self.sky, self.noise, dims_of(self.vol), what, planes)

    def done(self, what):
        self.frame(what)
        self.sc.destroy()


@BOTH
def test_inside_one_tile_and_through_each_face(vrt, oracle, engine, bricks):
    vol = np.zeros((24, 24, 24), np.uint8)
    vol[9:12, 10:13, 9:14] = 7                                             # inside the middle tile
    s = Scene(vrt, oracle, engine, vol, bricks)
    assert s.flood((10, 11, 10), 30, what="one tile")["region"] == 45
    assert s.sc.flood_rounds() == 1
    s.done("one tile")
    vol, seed, n = fc.plus_volume()
    s = Scene(vrt, oracle, engine, vol, bricks)
    assert s.flood(seed, 31, F.SOLID, 6, what="plus")["region"] == n
    assert s.flood((4, 12, 12), 32, F.SAME, 26, what="plus from an arm's end")["region"] == n
    s.done("plus")


@BOTH
@pytest.mark.parametrize("kind,a", list(itertools.product(("edge", "corner"), (8, 12))))
def test_diagonal_contact(vrt, oracle, engine, bricks, kind, a):
    vol, sa, sb = fc.diagonal_volume(kind, a)
    s = Scene(vrt, oracle, engine, vol, bricks)
    assert s.flood(sa, 33, F.SAME, 6, what="6 does not join")["region"] == 8
    assert s.flood(sb, 33, F.SOLID, 6, what="the other block")["region"] == 8
    assert s.flood(sb, 34, F.SAME, 26, what="26 joins")["region"] == 16
    s.done(f"{kind} {a}")


def test_maze_inside_one_tile(vrt, oracle, engine):
    vol, end, steps = fc.maze_volume(4)
    assert steps > 80
    s = Scene(vrt, oracle, engine, vol, False)
    assert s.flood(end, 3, F.SAME, 6, what="maze")["region"] == 127
    assert s.sc.flood_rounds() == 1                                         # one tile, one round: the fixed point is reached inside the step
    s.done("maze")


@BOTH
def test_serpentine_rounds_and_wakeups(vrt, oracle, engine, bricks):
    vol, first, mid, path = fc.serpentine_volume()
    s = Scene(vrt, oracle, engine, vol, bricks)
    assert s.flood(first, 2, what="from one end")["region"] == len(path)
    assert s.sc.flood_rounds() >= 12 * 2 + 2 + 1                            # a round per tile plane crossed, and the round that marks nothing
    assert s.flood(mid, 4, F.SOLID, 26, what="from the middle")["region"] == len(path)
    s.done("serpentine")
    cut = path[len(path) // 3]
    vol, first, mid, path = fc.serpentine_volume(cut=cut[:2])
    s = Scene(vrt, oracle, engine, vol, bricks)
    assert s.flood(first, 2, what="stops at the cut")["region"] == len(path) // 3
    assert s.flood(mid, 5, what="the rest, from the middle")["region"] == len(path) - len(path) // 3 - 1
    s.done("cut serpentine")


@BOTH
def test_bounds(vrt, oracle, engine, bricks):
    vol, inside, n = fc.cavity_volume()
    s = Scene(vrt, oracle, engine, vol, bricks)
    snap = bc.snapshot(vrt, s.sc, bricks)
    assert s.sc.flood(inside, 5, bounds=((100, 0, 0), (4, 4, 4))) == F.ZERO           # bounds wholly outside the volume
    assert s.sc.flood(inside, 5, bounds=((-9, -9, -9), (9, 9, 9))) == F.ZERO
    assert s.sc.flood(inside, 5, bounds=((0, 0, 0), (8, 8, 8))) == F.ZERO             # the seed outside the bounds
    assert s.sc.flood((-1, 3, 3), 5) == F.ZERO and s.sc.flood((40, 3, 3), 5) == F.ZERO
    assert bc.same_snapshot(snap, bc.snapshot(vrt, s.sc, bricks))
    assert s.flood(inside, 5, F.SAME, 6, ((8, 4, 6), (20, 14, 16)), "the leak stops at the bounds")["region"] == n + 1
    assert s.flood(inside, 0, F.SAME, 26, ((-4, -4, -4), (32, 40, 40)), "bounds partly outside, ending in the hole")["region"] == n + 1
    assert s.flood(inside, 6, F.SAME, 6, ((-4, -4, -4), (34, 40, 40)), "all the air of x < 30")["region"] == 30 * 24 * 32 - (20 * 14 * 16 - n - 1)
    s.done("cavity")


SCENES = [("dense-70x45x52", bc.DENSE_A, False, (11, 9, 13), (37, 30, 31)), ("dense-150x9x11", bc.DENSE_B, False, (21, 0, 1), (90, 9, 9)),
          ("bricks-9x6x7", bc.BRICKS, True, (13, 10, 9), (38, 29, 35))]


@pytest.mark.parametrize("name,dims,bricks,lo,size", SCENES, ids=[s[0] for s in SCENES])
def test_seeded_floods(vrt, oracle, engine, name, dims, bricks, lo, size):
    vol = bc.brick_volume(dims, 7) if bricks else bc.dense_volume(dims, sum(dims))
    half = (size[0] // 2, size[1], size[2])
    vol = fc.thin(vol, lo, half, fc.P6, 21)                                                  # one half near each threshold
    vol = fc.thin(vol, (lo[0] + half[0], lo[1], lo[2]), (size[0] - half[0], size[1], size[2]), fc.P26, 22)
    s = Scene(vrt, oracle, engine, vol, bricks, spare=400)
    regions = []
    for k, o in enumerate(fc.flood_sequence(vol, lo, size, 8, 31)):
        regions.append(s.flood(o["seed"], o["id"], o["match"], o["conn"], o["bounds"], f"{name} flood {k}")["region"])
    assert max(regions) > 100 and min(regions) == 0, regions
    s.done(name)


def test_noop_keeps_the_count_planes_fields(vrt, engine):
    dims = bc.DENSE_A
    W, H, D = dims
    vol = bc.dense_volume(dims, 5)
    vol[10:20, 10:20, 10:20] = 0
    vol[12:15, 12:15, 12:15] = 9
    pal = metallic_palette(vrt)
    sc = vrt.VoxelScene.from_dense(engine, vol, pal)
    st, push = bc.frame_setup(vrt, dims)
    vol, res = flood(vrt, engine, sc, vol, pal, False, (13, 13, 13), 10, F.SAME, 6, None, "a first flood")      # whatever a flood allocates is allocated
    assert res["changed"] == 27
    base = sc.memory_bytes()
    vrt.GeometryStage(engine, st, sc, debug_planes=True).record(push); engine.synchronize()     # count planes: the second set of fields
    held = sc.memory_bytes()
    assert held > base + W * H * D * 8
    snap = bc.snapshot(vrt, sc, False)
    for got, region in ((sc.flood((13, 13, 13), 10), 27), (sc.flood((13, 13, 13), 10, "solid", 26), 27), (sc.flood((11, 11, 11), 7, "solid"), 0),
                        (sc.flood((11, 11, 11), 0, "same", 6, ((10, 10, 10), (10, 10, 10))), 1000 - 27), (sc.flood((-5, 0, 0), 7), 0)):
        assert got["changed"] == 0 and got["lo"] == (0, 0, 0) and got["size"] == (0, 0, 0) and got["region"] == region, got
        assert sc.memory_bytes() == held and bc.same_snapshot(snap, bc.snapshot(vrt, sc, False))
    assert (bc.whole(sc, dims) == vol).all()
    assert sc.flood((13, 13, 13), 11)["changed"] == 27                       # a flood that writes drops them, as an edit does
    assert sc.memory_bytes() < held
    sc.trim()                                                                # ... and trim drops the flood's masks
    assert sc.memory_bytes() < base
    sc.destroy()


@pytest.mark.parametrize("kind", ["dense", "reserved", "unreserved"])
def test_measure(vrt, engine, kind):
    bricks = kind != "dense"
    dims = bc.BRICKS
    vol = np.zeros((dims[2], dims[1], dims[0]), np.uint8)
    vol[5:30, 7:20, 3:50] = 8; vol[10:20, 10:15, 10:40] = 0; vol[29:50, 12, 30] = 9             # one solid component, with a cavity
    pal = metallic_palette(vrt)
    sc = bc.make_scene(vrt, engine, vol, pal, bricks, spare=4 if kind == "reserved" else None)
    snap = bc.snapshot(vrt, sc, bricks)
    for seed, match, conn, bounds in (((4, 8, 6), "solid", 6, None), ((30, 12, 49), "solid", 26, None), ((4, 8, 6), "same", 6, None), ((12, 12, 12), "same", 6, None),
                                      ((0, 0, 0), "same", 26, None), ((0, 0, 0), "solid", 6, None), ((4, 8, 6), "solid", 6, ((-3, 2, 1), (20, 30, 22)))):
        got = sc.region(seed, match, conn, bounds)
        assert got == F.region(vol, seed, F.MATCHES[match], conn, bounds), (seed, match, conn, bounds, got)
    assert sc.region((4, 8, 6), "solid")[0] == sc.count((0, 0, 0), dims) == int((vol != 0).sum())    # the whole solid content is one component
    assert bc.same_snapshot(snap, bc.snapshot(vrt, sc, bricks))
    if kind == "unreserved":
        with pytest.raises(vrt._capi.VrtError) as err:
            sc.flood((4, 8, 6), 3)
        assert err.value.code == 7 and "vrt_scene_reserve_bricks" in str(err.value)
    sc.destroy()


def test_bricks_take_and_free_slots(vrt, oracle, engine):
    dims = bc.BRICKS
    vol = np.zeros((dims[2], dims[1], dims[0]), np.uint8)
    vol[4:44, 4:44, 4:60] = 8; vol[5:43, 5:43, 5:59] = 0                    # a closed shell around 6 x 4 x 4 whole bricks of air
    vol[48:56, 0:8, 0:16] = 9                                                # an object of two whole bricks
    need = int((~bc.brick_occupancy(vol) & bc.brick_occupancy(_filled(vol))).sum())      # the bricks of air the fill makes occupied
    assert need >= 10
    s = Scene(vrt, oracle, engine, vol, True, spare=need - 1)
    snap = bc.snapshot(vrt, s.sc, True)
    with pytest.raises(vrt._capi.VrtError) as err:
        s.sc.flood((20, 20, 20), 12)
    assert err.value.code == 7 and "vrt_scene_reserve_bricks" in str(err.value)
    assert bc.same_snapshot(snap, bc.snapshot(vrt, s.sc, True)) and (bc.whole(s.sc, dims) == vol).all()       # byte for byte as before
    assert s.flood((3, 3, 51), 0, F.SOLID, 6, what="delete the object: two bricks free their slots")["changed"] == 1024
    assert s.flood((20, 20, 20), 12, what="the cavity fill takes free slots")["region"] == 38 * 38 * 54
    s.done("bricks")


def _filled(vol):
    out = vol.copy()
    out[5:43, 5:43, 5:59] = 12
    return out


@BOTH
def test_metal_written_by_a_flood_is_seen(vrt, oracle, engine, bricks):
    dims = bc.BRICKS if bricks else bc.DENSE_A
    W, H, D = dims
    vol = bc.brick_volume(dims, 3) if bricks else bc.dense_volume(dims, 3)
    vol[0:2, :, :] = bc.ABSENT_ID                                                      # a wall facing the camera
    s = Scene(vrt, oracle, engine, vol, bricks)
    names = bc.GB + ["hit_id", "rays_total"]
    s.frame("before", names)
    assert s.sc.region((0, 0, 0), "same")[0] == 2 * W * H
    assert s.flood((0, 0, 0), bc.METAL_ID, what="metal")["changed"] == 2 * W * H
    exp = s.frame("after", names)
    assert (exp["hit_id"] == bc.METAL_ID).any() and int(exp["rays_total"].max()) > 6          # the mirror is seen, and bounces
    s.sc.destroy()


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_side_limit_512(vrt, engine, axis):
    dims = [9, 11, 9]
    dims[axis] = 520
    vol = np.zeros((dims[2], dims[1], dims[0]), np.uint8)
    line = [slice(4, 5), slice(3, 4), slice(2, 3)]
    line[2 - axis] = slice(0, 520)
    vol[tuple(line)] = 5
    pal = metallic_palette(vrt)
    sc = vrt.VoxelScene.from_dense(engine, vol, pal)
    lo, size, seed = [0, 0, 0], list(dims), [2, 3, 4]
    lo[axis], size[axis], seed[axis] = 4, 512, 4
    vol, res = flood(vrt, engine, sc, vol, pal, False, tuple(seed), 6, F.SAME, 6, (tuple(lo), tuple(size)), f"axis {axis}")
    assert res["region"] == 512 and res["size"][axis] == 512 and sc.flood_rounds() >= 64      # end to end: tile coordinate 63
    size[axis] = 513
    with pytest.raises(vrt._capi.VrtError) as err:
        sc.flood(tuple(seed), 7, bounds=(tuple(lo), tuple(size)))
    assert err.value.code == 1 and "flood in parts" in str(err.value)
    with pytest.raises(vrt._capi.VrtError):
        sc.region(tuple(seed))                                               # the whole volume is 520 long
    lo[axis], size[axis] = -7, 519                                           # 512 after the clip
    assert sc.region(tuple(seed), "solid", 26, (tuple(lo), tuple(size)))[0] == 512
    assert (bc.whole(sc, dims) == vol).all()
    sc.destroy()


def test_measure_512_cubed_bricks(vrt, engine):
    grid = np.zeros((64, 64, 64), np.uint32)
    where = [(0, 0, 0), (63, 63, 63), (31, 32, 33), (31, 32, 34), (5, 60, 17)]              # [z, y, x] of the occupied bricks
    for k, w in enumerate(where):
        grid[w] = k + 1
    pool = np.full((len(where), 8, 8, 8), 5, np.uint8)
    pool[4, 2:6, 2:6, 2:6] = 0                                               # a closed cavity: air the flood does not reach
    sc = vrt.VoxelScene.from_bricks(engine, grid, pool, metallic_palette(vrt))
    n, lo, size = sc.region((100, 100, 100), "same", 6)
    assert (n, lo, size) == (512 ** 3 - 512 * len(where), (0, 0, 0), (512, 512, 512))
    assert sc.region((17 * 8 + 3, 60 * 8 + 3, 5 * 8 + 3), "same", 26)[0] == 64
    assert sc.region((17 * 8, 60 * 8, 5 * 8), "solid", 6) == (512 - 64, (136, 480, 40), (8, 8, 8))
    assert sc.memory_bytes() > 2 * (16 << 20)                                # the two masks are counted
    sc.destroy()


def test_errors(vrt, engine):
    K, l = vrt._capi, vrt.lib()
    pal = metallic_palette(vrt)
    vol = bc.dense_volume((32, 24, 16), 2)
    sc = vrt.VoxelScene.from_dense(engine, vol, pal)

    def rc_of(match=0, conn=6, flags=0, size=(4, 4, 4), f=True, r=True, scene=True):
        fl = K.Flood(match=match, connectivity=conn, flags=flags, id=1)
        fl.seed[:], fl.lo[:], fl.size[:] = (1, 1, 1), (0, 0, 0), size
        res = K.FloodResult()
        rc = l.vrt_scene_flood(engine.ctx, sc.handle if scene else None, C.byref(fl) if f else None, C.byref(res) if r else None)
        return rc, l.vrt_last_error().decode()
    assert rc_of()[0] == 0
    vol, _ = F.flood(vol, (1, 1, 1), 1, bounds=((0, 0, 0), (4, 4, 4)))
    for kw in ({"match": 2}, {"match": -1}, {"conn": 18}, {"conn": 0}, {"flags": 2}, {"flags": 3}, {"size": (0, 4, 4)}, {"size": (4, 4, (1 << 30) + 1)},
               {"f": False}, {"r": False}, {"scene": False}):
        rc, msg = rc_of(**kw)
        assert rc == 1 and "vrt_scene_flood" in msg, (kw, rc, msg)
    assert (bc.whole(sc, (32, 24, 16)) == vol).all()
    with pytest.raises(ValueError):
        sc.flood((1, 1, 1), 256)
    sc.destroy()


@pytest.mark.parametrize("kind", sc_.KINDS)
def test_streams_behind_a_busy_device(vrt, kind):
    """an edit, then a flood that must see it, then a measure, on the HIP null stream, the context's own stream and a side stream of
    the caller, enqueued behind a stall with no synchronise by the caller in between; one synchronise at the end"""
    import torch
    dims = (40, 24, 32)
    vol = fc.random_volume(dims, 0.2, 51)
    pal = metallic_palette(vrt)
    side = torch.cuda.Stream() if kind == "side" else None
    with torch.cuda.stream(side if side is not None else torch.cuda.default_stream()):
        engine = vrt.Engine(0, use_torch_stream=kind != "own")
        lib, cap = vrt.lib(), vrt._capi
        scene = vrt.VoxelScene.from_dense(engine, vol, pal)
        stall_t, stall_p = None, C.c_void_p()
        if kind == "own":
            cap.check(lib.vrt_device_alloc(engine.ctx, sc_.STALL_BYTES, C.byref(stall_p)))
        else:
            stall_t = torch.zeros(sc_.STALL_BYTES // 4, dtype=torch.float32, device=engine.torch_device)
        torch.cuda.synchronize()
        for k in range(sc_.STALL_PASSES):                                 # the stall
            if kind == "own":
                cap.check(lib.vrt_memset(engine.ctx, stall_p, k, sc_.STALL_BYTES))
            else:
                stall_t.add_(1.0)
        scene.fill((5, 5, 5), (30, 3, 3), 44)                             # the edit the flood must see
        got1 = scene.flood((6, 6, 6), 45, "same", 26)
        got2 = scene.region((6, 6, 6), "solid", 6)
        read = scene.read((0, 0, 0), dims)
        engine.synchronize()
        if kind == "own":
            torch.cuda.synchronize()
            lib.vrt_device_free(engine.ctx, stall_p)
        v0 = vol.copy()
        v0[5:8, 5:8, 5:35] = 44
        v1, r1 = F.flood(v0, (6, 6, 6), 45, F.SAME, 26)
        assert r1["region"] == 270 and got1 == r1, kind
        assert got2 == F.region(v1, (6, 6, 6), F.SOLID, 6), kind
        assert (read == v1).all(), kind
        scene.destroy(); engine.destroy()
