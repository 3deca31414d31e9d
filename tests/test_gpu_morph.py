"""vrt_scene_morph on the GPU, held bit for bit to the reference (tests/morph_reference.py: r unit steps on the infinite grid, which
tests/test_morph_cpu.py proves equal to the closed form): every operation, connectivity and radius on a dense scene and on a
reserved brick scene with absent bricks, bounds around the row-word edges, clipped bounds, the halo, the volume's faces under
both border settings, known counts, the 512 limit, and the API's rules (no-op, MEASURE, bricks and their slots, metal, errors,
memory, streams).  After every call that changes something the scene's device structures equal a fresh build's; one small frame
per scene is held against the oracle."""
import ctypes as C
import itertools

import numpy as np
import pytest

import brush_common as bc
import morph_reference as M
import stream_common as sc_
import voxelize_common as vc
from helpers import metallic_palette
from morph_common import blobs

pytestmark = pytest.mark.gpu

BOTH = pytest.mark.parametrize("bricks", [False, True], ids=["dense", "bricks"])
OPS = (M.CLOSE, M.OPEN, M.HOLLOW, M.DILATE, M.ERODE)
NEW_ID = 77


def textures(vrt):
    return vrt.synthetic.sky_gradient(64, 32), vrt.synthetic.blue_noise_standin(64)


def dims_of(vol):
    return (vol.shape[2], vol.shape[1], vol.shape[0])


def morph(vrt, engine, sc, vol, pal, bricks, op, r, conn=6, vid=NEW_ID, bounds=None, border=False, what=""):
    """one operation on the scene and on the reference -> (the volume after, the result)"""
    exp_vol, exp = M.morph(vol, op, r, conn, vid, bounds, border)
    measured = sc.morph(op, r, conn, vid, bounds, border, measure=True)
    before = bc.snapshot(vrt, sc, bricks) if exp["changed"] == 0 else None
    got = sc.morph(op, r, conn, vid, bounds, border)
    print(what, op, r, conn, bounds, border, got)
    assert measured == dict(M.ZERO, added=exp["added"], removed=exp["removed"]), (what, measured, exp)
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

    def morph(self, op, r, conn=6, vid=NEW_ID, bounds=None, border=False, what=""):
        self.vol, res = morph(self.vrt, self.engine, self.sc, self.vol, self.pal, self.bricks, op, r, conn, vid, bounds, border, what)
        return res

    def frame(self, what, planes=bc.GB):
        return bc.assert_frame_equals_oracle(self.vrt, self.oracle, self.engine, self.sc, self.vol, self.pal, self.sky, self.noise, dims_of(self.vol), what, planes)

    def done(self, what):
        self.frame(what)
        self.sc.destroy()


def general_volume(bricks, seed):
    """blocks of 8^3 with pinholes; on the brick lattice an empty block is an absent brick"""
    return blobs(bc.BRICKS if bricks else bc.DENSE_A, seed, p=0.45, block=8, speckle=0.03, holes_only=bricks)


@BOTH
@pytest.mark.parametrize("conn,r", list(itertools.product((6, 26), (1, 3, 8))))
def test_every_operation_over_the_whole_volume(vrt, oracle, engine, bricks, conn, r):
    vol = general_volume(bricks, 40 + conn + r)
    if bricks:
        assert not bc.brick_occupancy(vol).all()
    s = Scene(vrt, oracle, engine, vol, bricks, spare=9 * 6 * 7)
    changed = [s.morph(op, r, conn, what=f"op {op}")["changed"] for op in OPS]
    assert sum(1 for c in changed if c) >= 3, changed
    s.done(f"whole volume {conn} {r}")


@BOTH
def test_bounds_around_the_row_word_edges(vrt, oracle, engine, bricks):
    dims = (136, 16, 16) if bricks else bc.DENSE_B
    W, H, D = dims
    vol = blobs(dims, 9, p=0.5, block=8 if bricks else 3, holes_only=bricks)
    s = Scene(vrt, oracle, engine, vol, bricks, spare=17 * 2 * 2)
    k = 0
    for x0, x1 in itertools.product((63, 64, 65), repeat=2):                 # the x range starts at x0 and ends at x1, or spans them
        op = (M.DILATE, M.OPEN, M.HOLLOW, M.ERODE, M.CLOSE)[k % 5]
        k += 1
        s.morph(op, 2, 26 if k % 2 else 6, bounds=((x0, 0, 0), (W - x0, H, D)), what=f"from {x0}")
        s.morph(op, 1, 6 if k % 2 else 26, bounds=((0, 1, 1), (x1, H, D)), what=f"to {x1}")
        if x1 > x0:
            s.morph(M.DILATE, 1, 6, NEW_ID + k, bounds=((x0, 2, 3), (x1 - x0, 5, 5)), what=f"{x0} to {x1}")
    s.done("row words")


@BOTH
def test_clipped_bounds_and_bounds_outside(vrt, oracle, engine, bricks):
    vol = general_volume(bricks, 3)
    W, H, D = dims_of(vol)
    s = Scene(vrt, oracle, engine, vol, bricks, spare=200)
    snap = bc.snapshot(vrt, s.sc, bricks)
    assert s.sc.morph("dilate", 2, 6, 5, bounds=((W, 0, 0), (4, 4, 4))) == M.ZERO          # wholly outside the volume
    assert s.sc.morph("erode", 8, 26, bounds=((-9, -9, -9), (9, 9, 9))) == M.ZERO
    assert bc.same_snapshot(snap, bc.snapshot(vrt, s.sc, bricks))
    s.morph(M.DILATE, 2, 6, bounds=((-5, -7, -3), (30, 25, 20)), what="clipped by three low faces")
    s.morph(M.ERODE, 1, 26, bounds=((W - 20, H - 11, D - 13), (1 << 30, 100, 50)), border=True, what="clipped by three high faces")
    s.morph(M.CLOSE, 3, 6, bounds=((-(1 << 31), 10, -2), ((1 << 30), 9, 12)), what="lo at the int32 edge: nothing left")
    s.morph(M.OPEN, 2, 26, bounds=((-100, 5, 5), (100 + W + 100, 20, 20)), what="through the volume")
    s.done("clipped")


@BOTH
@pytest.mark.parametrize("r", [1, 3])
def test_the_halo_is_read_and_nothing_beyond_it(vrt, oracle, engine, bricks, r):
    """bounds of 9^3 strictly inside, single solids exactly r, r + 1, 2r and 2r + 1 cells outside them, one per face and distance"""
    dims = (40, 40, 40)
    lo, size = (15, 16, 14), (9, 9, 9)
    base = np.zeros((40, 40, 40), np.uint8)
    base[18:21, 19:22, 17:20] = 9                                            # a 3^3 block inside the bounds
    if bricks:
        base[0:8, 0:8, 0:8] = 4                                              # so that far bricks exist and most are absent
    ds = (r, r + 1, 2 * r, 2 * r + 1)
    for k, d in enumerate(ds):
        vol = base.copy()
        c = [lo[a] + 4 for a in range(3)]
        for a in range(3):
            for far in (0, 1):
                p = list(c)
                p[a] = lo[a] + size[a] - 1 + d if far else lo[a] - d
                p[(a + 1) % 3] += k - 1                                        # (off the centre line, differently per distance)
                vol[p[2], p[1], p[0]] = 30 + a
        vol[lo[2] - 1, lo[1] - 1, lo[0] - d] = 33                            # diagonally off a corner: 26 sees farther than 6
        s = Scene(vrt, oracle, engine, vol, bricks, spare=100)
        for op, conn in itertools.product((M.DILATE, M.CLOSE, M.ERODE, M.OPEN, M.HOLLOW), (6, 26)):
            s.morph(op, r, conn, bounds=(lo, size), border=(op + k) % 2 == 1, what=f"d {d} op {op} conn {conn}")
        assert (s.vol[~_inside(dims, lo, size)] == vol[~_inside(dims, lo, size)]).all()
        s.done(f"halo {r} {d}")


def _inside(dims, lo, size):
    m = np.zeros((dims[2], dims[1], dims[0]), bool)
    m[lo[2]:lo[2] + size[2], lo[1]:lo[1] + size[1], lo[0]:lo[0] + size[0]] = True
    return m


@BOTH
def test_slabs_on_the_volume_faces_under_both_borders(vrt, oracle, engine, bricks):
    dims = (24, 16, 32)
    W, H, D = dims
    for a, far in itertools.product(range(3), (0, 1)):
        vol = np.zeros((D, H, W), np.uint8)
        sl = [slice(None)] * 3
        sl[2 - a] = slice(dims[a] - 3, dims[a]) if far else slice(0, 3)
        vol[tuple(sl)] = 12 + a
        for op, border in itertools.product((M.ERODE, M.HOLLOW), (False, True)):
            s = Scene(vrt, oracle, engine, vol, bricks, spare=10)
            res = s.morph(op, 1, 6, border=border, what=f"face {a}{'+' if far else '-'} op {op} border {border}")
            s.morph(op, 2, 26, border=border, what="again, wider")
            # with the border solid the slab is eroded from its free side only and its rim stays; with it empty from both sides
            n = dims[(a + 1) % 3] * dims[(a + 2) % 3]
            assert res["removed"] == ({M.ERODE: n, M.HOLLOW: 2 * n}[op] if border else {M.ERODE: 3 * n - max(0, (dims[(a + 1) % 3] - 2) * (dims[(a + 2) % 3] - 2)), M.HOLLOW: max(0, (dims[(a + 1) % 3] - 2) * (dims[(a + 2) % 3] - 2))}[op]), res
            s.sc.destroy()


def test_known_counts(vrt, oracle, engine):
    for conn, n in ((6, 833), (26, 17 ** 3)):
        vol = np.zeros((21, 19, 23), np.uint8)
        vol[10, 9, 11] = 5
        s = Scene(vrt, oracle, engine, vol, False)
        assert s.morph(M.DILATE, 8, conn)["added"] == n - 1
        assert int((bc.whole(s.sc, (23, 19, 21)) != 0).sum()) == n            # the octahedron; the cube
        assert s.sc.count((0, 0, 0), (23, 19, 21)) == n
        s.done(f"single voxel {conn}")


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_side_limit_512(vrt, engine, axis):
    dims = [9, 9, 9]
    dims[axis] = 530
    vol = blobs(tuple(dims), 60 + axis, p=0.7, block=9, speckle=0.01)
    pal = metallic_palette(vrt)
    sc = vrt.VoxelScene.from_dense(engine, vol, pal)
    lo, size = [0, 0, 0], list(dims)
    lo[axis], size[axis] = 9, 512
    vol, res = morph(vrt, engine, sc, vol, pal, False, M.OPEN, 8, 26, 0, (tuple(lo), tuple(size)), True, f"axis {axis}")    # the domain is 544 long
    assert res["removed"] > 0 and res["added"] == 0
    size[axis] = 513
    with pytest.raises(vrt._capi.VrtError) as err:
        sc.open(8, 26, bounds=(tuple(lo), tuple(size)))
    assert err.value.code == 1 and "work in parts" in str(err.value)
    with pytest.raises(vrt._capi.VrtError):
        sc.hollow(1, measure=True)                                           # the whole volume is 530 long
    lo[axis], size[axis] = -7, 519                                           # 512 after the clip
    vol, res = morph(vrt, engine, sc, vol, pal, False, M.HOLLOW, 1, 6, 0, (tuple(lo), tuple(size)), False, "clipped to 512")
    assert res["size"][axis] <= 512
    sc.destroy()


def test_noop_keeps_the_count_planes_fields(vrt, engine):
    dims = bc.DENSE_A
    W, H, D = dims
    vol = blobs(dims, 5, p=0.4, block=6, speckle=0.02)
    vol[10:20, 10:20, 10:20] = 0
    pal = metallic_palette(vrt)
    sc = vrt.VoxelScene.from_dense(engine, vol, pal)
    st, push = bc.frame_setup(vrt, dims)
    vol, res = morph(vrt, engine, sc, vol, pal, False, M.OPEN, 1, 6, 0, None, False, "a first opening")       # whatever a call allocates is allocated
    assert res["removed"] > 0
    base = sc.memory_bytes()
    vrt.GeometryStage(engine, st, sc, debug_planes=True).record(push); engine.synchronize()     # count planes: the second set of fields
    held = sc.memory_bytes()
    assert held > base + W * H * D * 8
    snap = bc.snapshot(vrt, sc, False)
    for got in (sc.open(1, 6), sc.erode(2, 26, bounds=((11, 11, 11), (8, 8, 8))), sc.hollow(8, 6, bounds=((10, 10, 10), (10, 10, 10))),
                sc.dilate(1, 9, 6, bounds=((13, 13, 13), (4, 4, 4))), sc.erode(1, bounds=((-5, 0, 0), (5, 9, 9)))):
        assert got == M.ZERO, got
        assert sc.memory_bytes() == held and bc.same_snapshot(snap, bc.snapshot(vrt, sc, False))
    assert (bc.whole(sc, dims) == vol).all()
    assert sc.hollow(1)["removed"] > 0                                       # a call that writes drops them, as an edit does
    assert sc.memory_bytes() < held
    with_masks = sc.memory_bytes()
    sc.trim()                                                                # ... and trim drops the masks
    words = -(-(W + 2) // 32) * (H + 2) * (D + 2)
    assert sc.memory_bytes() <= with_masks - 2 * 4 * words
    sc.destroy()


@pytest.mark.parametrize("kind", ["dense", "reserved", "unreserved"])
def test_measure(vrt, engine, kind):
    bricks = kind != "dense"
    vol = general_volume(True, 8)
    pal = metallic_palette(vrt)
    sc = bc.make_scene(vrt, engine, vol, pal, bricks, spare=4 if kind == "reserved" else None)
    snap = bc.snapshot(vrt, sc, bricks)
    m0 = sc.memory_bytes()
    assert sc.hollow(1, measure=True)["removed"] > 0
    W, H, D = bc.BRICKS
    assert sc.memory_bytes() >= m0 + 2 * 4 * (-(-(W + 2) // 32) * (H + 2) * (D + 2))      # vrt_scene_memory grows by the two masks
    sc.trim()
    assert sc.memory_bytes() == m0                                           # ... and vrt_scene_trim returns them
    for op, r, conn, bounds, border in ((M.DILATE, 1, 6, None, False), (M.ERODE, 2, 26, None, True), (M.OPEN, 3, 6, ((-3, 2, 1), (40, 30, 22)), False),
                                        (M.CLOSE, 8, 26, ((20, 8, 8), (30, 30, 30)), False), (M.HOLLOW, 1, 6, None, True)):
        exp = M.morph(vol, op, r, conn, 5, bounds, border, measure=True)[1]
        assert sc.morph(op, r, conn, 5, bounds, border, measure=True) == exp, (op, r, conn)
    assert bc.same_snapshot(snap, bc.snapshot(vrt, sc, bricks))
    if kind == "unreserved":
        with pytest.raises(vrt._capi.VrtError) as err:
            sc.hollow(1)
        assert err.value.code == 7 and "vrt_scene_reserve_bricks" in str(err.value)
        assert bc.same_snapshot(snap, bc.snapshot(vrt, sc, bricks))
    sc.destroy()


def test_bricks_take_and_free_slots(vrt, oracle, engine):
    dims = bc.BRICKS
    vol = np.zeros((dims[2], dims[1], dims[0]), np.uint8)
    vol[8:40, 8:40, 8:56] = 8                                                # 6 x 4 x 4 whole bricks
    need = int((bc.brick_occupancy(M.morph(vol, M.DILATE, 1, 26, 12)[0]) & ~bc.brick_occupancy(vol)).sum())      # the shell of bricks around them
    assert need == 8 * 6 * 6 - 6 * 4 * 4
    s = Scene(vrt, oracle, engine, vol, True, spare=need - 1)
    snap = bc.snapshot(vrt, s.sc, True)
    with pytest.raises(vrt._capi.VrtError) as err:
        s.sc.dilate(1, 12, 26)
    assert err.value.code == 7 and "vrt_scene_reserve_bricks" in str(err.value)
    assert bc.same_snapshot(snap, bc.snapshot(vrt, s.sc, True)) and (bc.whole(s.sc, dims) == vol).all()       # byte for byte as before
    assert s.morph(M.ERODE, 8, 6, what="bricks vanish and free their slots")["removed"] > 0
    assert s.morph(M.DILATE, 1, 26, 12, what="the dilation takes free slots")["added"] > 0
    s.done("bricks")


@BOTH
def test_metal_written_by_a_dilation_is_seen(vrt, oracle, engine, bricks):
    dims = bc.BRICKS if bricks else bc.DENSE_A
    vol = bc.brick_volume(dims, 3) if bricks else bc.dense_volume(dims, 3)
    vol[0:2, :, :] = 0
    vol[2:4, :, :] = bc.ABSENT_ID                                                      # a wall, two voxels behind the face the camera looks at
    s = Scene(vrt, oracle, engine, vol, bricks, spare=200)
    names = bc.GB + ["hit_id", "rays_total"]
    s.frame("before", names)
    assert s.morph(M.DILATE, 1, 6, bc.METAL_ID, bounds=((0, 0, 0), (dims[0], dims[1], 3)), what="metal")["added"] >= dims[0] * dims[1]
    exp = s.frame("after", names)
    assert (exp["hit_id"] == bc.METAL_ID).any() and int(exp["rays_total"].max()) > 6          # the mirror is seen, and bounces
    s.sc.destroy()


def test_errors(vrt, engine):
    K, l = vrt._capi, vrt.lib()
    pal = metallic_palette(vrt)
    vol = bc.dense_volume((32, 24, 16), 2)
    sc = vrt.VoxelScene.from_dense(engine, vol, pal)

    def rc_of(op=M.DILATE, conn=6, radius=1, flags=0, vid=1, size=(4, 4, 4), m=True, r=True, scene=True):
        mo = K.Morph(op=op, connectivity=conn, radius=radius, flags=flags, id=vid)
        mo.lo[:], mo.size[:] = (0, 0, 0), size
        res = K.MorphResult()
        rc = l.vrt_scene_morph(engine.ctx, sc.handle if scene else None, C.byref(mo) if m else None, C.byref(res) if r else None)
        return rc, l.vrt_last_error().decode()
    assert rc_of()[0] == 0
    vol, _ = M.morph(vol, M.DILATE, 1, 6, 1, ((0, 0, 0), (4, 4, 4)))
    for kw in ({"op": 5}, {"op": -1}, {"conn": 18}, {"conn": 0}, {"radius": 0}, {"radius": 9}, {"radius": -1}, {"flags": 4}, {"flags": 7}, {"vid": 0},
               {"op": M.CLOSE, "vid": 0}, {"size": (0, 4, 4)}, {"size": (4, 4, (1 << 30) + 1)}, {"m": False}, {"r": False}, {"scene": False}):
        rc, msg = rc_of(**kw)
        assert rc == 1 and "vrt_scene_morph" in msg, (kw, rc, msg)
    for op in (M.ERODE, M.OPEN, M.HOLLOW):
        assert rc_of(op=op, vid=0, flags=2)[0] == 0                          # they ignore the id
    assert (bc.whole(sc, (32, 24, 16)) == vol).all()
    with pytest.raises(ValueError):
        sc.dilate(1, 256)
    with pytest.raises(KeyError):
        sc.morph("thicken", 1)
    sc.destroy()


@pytest.mark.parametrize("kind", sc_.KINDS)
def test_streams_behind_a_busy_device(vrt, kind):
    """an edit, then an operation that must see it, then a measure, on the HIP null stream, the context's own stream and a side
    stream of the caller, enqueued behind a stall with no synchronise by the caller in between; one synchronise at the end"""
    import torch
    dims = (40, 24, 32)
    vol = blobs(dims, 51, p=0.3, block=4)
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
        scene.fill((5, 5, 5), (30, 9, 9), 44)                             # the edit the operation must see
        got1 = scene.hollow(2, 26)
        got2 = scene.dilate(1, 45, 6, measure=True)
        read = scene.read((0, 0, 0), dims)
        engine.synchronize()
        if kind == "own":
            torch.cuda.synchronize()
            lib.vrt_device_free(engine.ctx, stall_p)
        v0 = vol.copy()
        v0[5:14, 5:14, 5:35] = 44
        v1, r1 = M.morph(v0, M.HOLLOW, 2, 26)
        assert r1["removed"] >= 26 * 5 * 5 and got1 == r1, kind
        assert got2 == M.morph(v1, M.DILATE, 1, 6, 45, measure=True)[1], kind
        assert (read == v1).all(), kind
        scene.destroy(); engine.destroy()


@BOTH
def test_hollow_a_voxelized_solid(vrt, oracle, engine, bricks):
    """voxelize a closed mesh SOLID, hollow it to a shell one voxel thick: the closed face count gains the cavity's faces and the
    view from outside does not change"""
    dims = (48, 40, 40)
    vol = np.zeros((40, 40, 48), np.uint8)
    vol[0, 0, 0] = 3
    s = Scene(vrt, oracle, engine, vol, bricks, spare=200)
    v, t = vc.sphere_mesh((24.0, 20.0, 20.0), 13.0)
    res = s.sc.voxelize(v, t, 21, "set", "solid")
    assert res["changed"] > 2000
    s.vol = bc.whole(s.sc, dims)
    solid = s.vol.copy()
    faces0 = int(s.sc.face_count((0, 0, 0), dims, closed=True).sum())
    before = s.frame("the solid")
    res = s.morph(M.HOLLOW, 1, 6, what="hollow")
    assert res["removed"] > 500 and res["added"] == 0
    faces1 = int(s.sc.face_count((0, 0, 0), dims, closed=True).sum())
    assert faces1 > faces0, (faces0, faces1)                                 # the cavity's faces
    after = s.frame("the shell")
    for n in bc.GB:
        assert (np.asarray(before[n]) == np.asarray(after[n])).all(), n       # the outside view is unchanged
    assert s.sc.region((24, 20, 20), "same", 6)[0] == res["removed"]         # one closed cavity: what was removed
    assert ((s.vol != 0) <= (solid != 0)).all()
    s.sc.destroy()


def test_app_morph_in_order_then_save(vrt, oracle, tmp_path):
    """vrt_app --fill ... --morph hollow:6:1 --morph dilate:... --save-vox OUT (the C++ mirror's VoxelScene::morph): the saved file
    loads -- with the library's loader and, where it is built, the reference's -- to the volume the reference composes"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    app = os.path.join(root, "voxel-raytracing_amd", "host", "vrt_app")
    assert os.path.exists(app), "build with __graft_entry__.build()"
    path = os.path.join(root, "tests", "golden", "vox_multi.vox")
    vol = vrt.vox_flatten_host(open(path, "rb").read())[0].copy()
    D, H, W = vol.shape
    sx, sy, sz = max(1, W - 2), max(1, H - 2), max(1, D - 2)
    out = tmp_path / "shell.vox"
    args = ["--fill", "1", "1", "1", str(sx), str(sy), str(sz), "7", "--morph", "hollow:6:1",
            "--morph", f"dilate:26:1:9:solid:-3,0,0:{W + 1},{H},{max(1, D // 2)}"]
    p = subprocess.run([app, "--vox", path] + args + ["--save-vox", str(out)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    vol[1:1 + sz, 1:1 + sy, 1:1 + sx] = 7
    vol, r1 = M.morph(vol, M.HOLLOW, 1, 6)
    vol, r2 = M.morph(vol, M.DILATE, 1, 26, 9, ((-3, 0, 0), (W + 1, H, max(1, D // 2))), True)
    assert f"morph: 0 voxels added, {r1['removed']} removed" in p.stdout and f"morph: {r2['added']} voxels added, 0 removed" in p.stdout, p.stdout
    data = out.read_bytes()
    got = vrt.vox_flatten_host(data)[0]
    assert got.shape == vol.shape and (got == vol).all()
    if oracle.refvox() is not None:
        r, rvox, _, _, dropped = oracle.refvox_flatten(data)
        assert r == 0 and dropped == 0 and rvox.shape == vol.shape and (rvox == vol).all()
    bad = subprocess.run([app, "--vox", path, "--morph", "dilate:6:1", "--save-vox", str(out)], capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "id != 0" in bad.stderr
    bad = subprocess.run([app, "--vox", path, "--morph", "thicken:6:1"], capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "unknown operation" in bad.stderr
