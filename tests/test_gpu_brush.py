"""vrt_scene_brush on the GPU: a seeded sequence of brushes on two awkward dense scenes and a reserved brick scene.  After every
brush the result equals the reference's (tests/brush_reference.py, Python integers) and the whole volume read back equals the
numpy volume; the scene's device structures equal a fresh build's; every fifth brush a small frame equals the oracle's; a no-op
leaves every byte and the count planes' fields alone; errors; three kinds of stream behind a busy device."""
import ctypes as C

import numpy as np
import pytest

import brush_common as bc
import brush_reference as R
import stream_common as sc_
from helpers import metallic_palette

pytestmark = pytest.mark.gpu

SCENES = [("dense-70x45x52", bc.DENSE_A, False), ("dense-150x9x11", bc.DENSE_B, False), ("bricks-9x6x7", bc.BRICKS, True)]


@pytest.mark.parametrize("name,dims,bricks", SCENES, ids=[s[0] for s in SCENES])
def test_sequence_of_brushes(vrt, oracle, engine, name, dims, bricks):
    K = vrt._capi
    vol = bc.brick_volume(dims, 7) if bricks else bc.dense_volume(dims, sum(dims))
    pal = metallic_palette(vrt)
    assert not (vol >= 200).any() and not (vol == bc.ABSENT_ID).any() and (vol == bc.BLOCK_ID).any()
    sky, noise = vrt.synthetic.sky_gradient(64, 32), vrt.synthetic.blue_noise_standin(64)
    sc = bc.make_scene(vrt, engine, vol, pal, bricks, sky=sky, noise=noise)
    cap = int(bc.brick_occupancy(vol).sum()) + bc.BRICK_SPARE if bricks else 0
    seq = bc.brush_sequence(dims, 11)
    assert len(seq) >= 40
    seen = {"no-op": 0, "refused": [], "clipped": 0, "appear": 0, "vanish": 0}
    spans = set()
    for k, o in enumerate(seq):
        what = f"{name} brush {k} ({o['kind']})"
        free = cap - int(bc.brick_occupancy(vol).sum()) if bricks else 0
        exp, res, refused = bc.expected(vol, o, bricks, free)
        noop = res[0] == 0
        before = bc.snapshot(vrt, sc, bricks) if noop else None
        if refused:
            with pytest.raises(K.VrtError) as err:
                sc.brush(o["shape"], o["mode"], o["p"], o["id"], o["match"])
            assert err.value.code == 7 and "vrt_scene_reserve_bricks" in str(err.value), what
            seen["refused"].append(o["kind"])
        else:
            got = sc.brush(o["shape"], o["mode"], o["p"], o["id"], o["match"])
            print(what, got)
            assert got == (res[0], tuple(res[1]), tuple(res[2])), (what, got, res)
        if o["kind"].startswith("no-op"):
            assert noop, what
        if noop:
            seen["no-op"] += 1
            assert bc.same_snapshot(before, bc.snapshot(vrt, sc, bricks)), what      # byte-identical, slot assignment included
        if bricks and not noop:
            occ0, occ1 = bc.brick_occupancy(vol), bc.brick_occupancy(exp)
            seen["appear"] += int((occ1 & ~occ0).any()); seen["vanish"] += int((occ0 & ~occ1).any())
        lo, hi = R.bounds(o["shape"], o["p"])
        c = R.clip(lo, hi, dims)
        if c is not None:
            seen["clipped"] += int(any(lo[a] < 0 or hi[a] > dims[a] for a in range(3)))
            if c[0][0] % 2 == 1:
                spans.add((c[1][0] + 63) // 64)
        vol = exp
        assert (bc.whole(sc, dims) == vol).all(), what
        if not bricks or k % 4 == 3 or k == len(seq) - 1:
            bc.assert_state_equals_fresh(vrt, engine, sc, vol, pal, bricks, what)
        if k % 5 == 4 or o["id"] == bc.METAL_ID:
            bc.assert_frame_equals_oracle(vrt, oracle, engine, sc, vol, pal, sky, noise, dims, what)
    assert seen["no-op"] >= 7 and seen["clipped"] >= 8, seen
    assert spans >= ({1, 2, 3} if dims[0] > 128 else {1, 2}), spans
    if bricks:
        assert "needs more slots" in seen["refused"] and len(seen["refused"]) <= 3 and seen["appear"] >= 2 and seen["vanish"] >= 2, seen
    assert (vol == bc.METAL_ID).sum() == 0 and (vol == 72).any()             # the metal was painted over: the scene stays one whose rays may bounce
    sc.destroy()


@pytest.mark.parametrize("bricks", [False, True], ids=["dense", "bricks"])
def test_metal_written_by_a_brush_is_seen(vrt, oracle, engine, bricks):
    """a scene without a metallic voxel renders through the kernel without the bounce loop; a brush that writes one changes that:
    the rays-per-pixel plane shows bounces, and every plane equals the oracle's"""
    dims = bc.BRICKS if bricks else bc.DENSE_A
    W, H, D = dims
    vol = bc.brick_volume(dims, 3) if bricks else bc.dense_volume(dims, 3)
    pal = metallic_palette(vrt)
    sky, noise = vrt.synthetic.sky_gradient(64, 32), vrt.synthetic.blue_noise_standin(64)
    sc = bc.make_scene(vrt, engine, vol, pal, bricks, sky=sky, noise=noise, spare=64)
    names = bc.GB + ["hit_id", "rays_total"]
    bc.assert_frame_equals_oracle(vrt, oracle, engine, sc, vol, pal, sky, noise, dims, "before", names)
    # a metallic brush that writes nothing
    assert sc.sphere((W / 2, H / 2, -30.0), 4.0, bc.METAL_ID, "paint")[0] == 0
    p = [0, 0, 0, W, H, 2]
    vol, res = R.brush(vol, R.BOX, R.SET, p, bc.METAL_ID)
    assert sc.box(p[:3], p[3:], bc.METAL_ID) == (res[0], tuple(res[1]), tuple(res[2]))
    exp = bc.assert_frame_equals_oracle(vrt, oracle, engine, sc, vol, pal, sky, noise, dims, "after", names)
    assert (exp["hit_id"] == bc.METAL_ID).any() and int(exp["rays_total"].max()) > 6          # the mirror is seen, and bounces
    sc.destroy()


def test_noop_keeps_the_count_planes_fields(vrt, engine):
    dims = bc.DENSE_A
    W, H, D = dims
    vol = bc.dense_volume(dims, 5)
    vol[10:20, 10:20, 10:20] = 0
    pal = metallic_palette(vrt)
    sc = vrt.VoxelScene.from_dense(engine, vol, pal)
    st, push = bc.frame_setup(vrt, dims)
    sc.sphere((1.5, 1.5, 1.5), 1.0, 9)                                       # a first brush: whatever a brush allocates is allocated
    vol, _ = R.brush(vol, R.ELLIPSOID, R.SET, bc.sphere((1.5, 1.5, 1.5), 1.0), 9)
    base = sc.memory_bytes()
    vrt.GeometryStage(engine, st, sc, debug_planes=True).record(push); engine.synchronize()     # count planes: the second set of fields
    held = sc.memory_bytes()
    assert held > base + W * H * D * 8
    snap = bc.snapshot(vrt, sc, False)
    for got in (sc.sphere((15.0, 15.0, 15.0), 3.0, 7, "paint"), sc.box((0, 0, 0), dims, 8, "replace", match=bc.ABSENT_ID), sc.sphere((1.5, 1.5, 1.5), 1.0, 9),
                sc.sphere((-30.0, 5.0, 5.0), 4.0, 7), sc.box((W, 0, 0), (3, 3, 3), 7)):
        assert got == (0, (0, 0, 0), (0, 0, 0))
        assert sc.memory_bytes() == held and bc.same_snapshot(snap, bc.snapshot(vrt, sc, False))
    assert (bc.whole(sc, dims) == vol).all()
    assert sc.sphere((15.0, 15.0, 15.0), 3.0, 7)[0] > 0                      # a brush that writes drops them, as an edit does
    assert sc.memory_bytes() < held
    sc.destroy()


def test_errors(vrt, engine):
    K, l = vrt._capi, vrt.lib()
    pal = metallic_palette(vrt)
    vol = bc.dense_volume((32, 24, 16), 2)
    sc = vrt.VoxelScene.from_dense(engine, vol, pal)

    def rc_of(shape, mode, p, vid=1, match=0, scene=None, res=True):
        b = K.Brush(shape=shape, mode=mode, id=vid, match=match)
        b.p[:len(p)] = p
        r = K.BrushResult()
        rc = l.vrt_scene_brush(engine.ctx, (scene or sc).handle, C.byref(b), C.byref(r) if res else None)
        return rc, l.vrt_last_error().decode()
    ok = [10, 10, 10, 4, 4, 4, 3]
    for shape, mode, p, vid, match in ((3, R.SET, ok, 1, 0), (-1, R.SET, ok, 1, 0), (R.BOX, 4, ok, 1, 0), (R.BOX, -1, ok, 1, 0),
                                       (R.ELLIPSOID, R.SET, [10, 10, 10, 0, 4, 4], 1, 0), (R.ELLIPSOID, R.SET, [10, 10, 10, 4, 1025, 4], 1, 0),
                                       (R.CAPSULE, R.SET, [10, 10, 10, 4, 4, 4, 0], 1, 0), (R.CAPSULE, R.SET, [10, 10, 10, 4, 4, 4, 1025], 1, 0),
                                       (R.CAPSULE, R.SET, [-4097, 10, 10, 4, 4, 4, 3], 1, 0), (R.CAPSULE, R.SET, [10, 10, 10, 4, 12289, 4, 3], 1, 0),
                                       (R.BOX, R.SET, [0, 0, 0, 4, 0, 4], 1, 0), (R.BOX, R.SET, [0, 0, 0, 4, -2, 4], 1, 0),
                                       (R.BOX, R.PAINT, ok, 0, 0), (R.BOX, R.ADD, ok, 0, 5), (R.BOX, R.REPLACE, ok, 5, 5)):
        rc, msg = rc_of(shape, mode, p, vid, match)
        assert rc == 1 and "vrt_scene_brush" in msg, (shape, mode, p, vid, match, rc, msg)
    assert (bc.whole(sc, (32, 24, 16)) == vol).all()                          # a refused brush changes nothing
    assert rc_of(R.ELLIPSOID, R.SET, [10, 10, 10, 4, 4, 4], res=False)[0] == 0            # result may be NULL
    vol, _ = R.brush(vol, R.ELLIPSOID, R.SET, [10, 10, 10, 4, 4, 4], 1)
    assert (bc.whole(sc, (32, 24, 16)) == vol).all()
    with pytest.raises(ValueError):
        sc.sphere((1.25, 2, 2), 1.0, 3)                                       # not a multiple of 0.5
    with pytest.raises(ValueError):
        sc.capsule((1, 2, 2), (3, 3, 3), 0.75, 3)
    sc.destroy()
    grid = np.zeros((2, 3, 4), np.uint32); grid[1, 1, 1] = 1
    bs = vrt.VoxelScene.from_bricks(engine, grid, np.full((1, 8, 8, 8), 5, np.uint8), pal)
    rc, msg = rc_of(R.BOX, R.SET, ok, scene=bs)
    assert rc == 7 and "vrt_scene_brush" in msg and "vrt_scene_reserve_bricks" in msg  # the edit's words
    assert rc_of(R.BOX, R.SET, [0, 0, 0, 0, 1, 1], scene=bs)[0] == 1                    # arguments first
    bs.reserve_bricks(2)
    assert bs.box((8, 8, 8), (8, 8, 8), 0) == (512, (8, 8, 8), (8, 8, 8))                   # carves the one brick away
    assert bs.count((0, 0, 0), (32, 24, 16)) == 0
    assert bs.sphere((4.0, 4.0, 4.0), 2.0, 6, "add")[0] > 0
    bs.destroy()


@pytest.mark.parametrize("kind", sc_.KINDS)
def test_streams_behind_a_busy_device(vrt, kind):
    """one brush and one stamp on the HIP null stream, the context's own stream and a side stream of the caller, enqueued behind a
    stall with no synchronise by the caller in between; one synchronise at the end"""
    import torch
    dims = (40, 24, 32)
    rng = np.random.default_rng(51)
    vol = ((rng.random((32, 24, 40)) < 0.2) * rng.integers(1, 199, (32, 24, 40))).astype(np.uint8)
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
        p = bc.sphere((20.5, 12.0, 16.5), 6.5)
        got1 = scene.brush(R.ELLIPSOID, R.ADD, p, 77)
        got2 = scene.stamp((-2, 3, 20), scene, (10, 4, 6), (17, 9, 11), orient=3 | 5 << 3, skip_empty=True)
        read = scene.read((0, 0, 0), dims)
        engine.synchronize()
        if kind == "own":
            torch.cuda.synchronize()
            lib.vrt_device_free(engine.ctx, stall_p)
        v1, r1 = R.brush(vol, R.ELLIPSOID, R.ADD, p, 77)
        v2, r2 = R.stamp(v1, (-2, 3, 20), v1, (10, 4, 6), (17, 9, 11), 3 | 5 << 3, True)
        assert r1[0] > 0 and r2[0] > 0
        assert got1 == (r1[0], tuple(r1[1]), tuple(r1[2])) and got2 == (r2[0], tuple(r2[1]), tuple(r2[2])), kind
        assert (read == v2).all(), kind
        scene.destroy(); engine.destroy()
