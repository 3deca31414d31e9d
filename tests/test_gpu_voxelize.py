"""vrt_scene_voxelize on the GPU, held bit for bit to the definition in Python integers (tests/voxelize_reference.py).  After every
call the result dict, the whole volume and `covered` equal the reference; when something changed the scene's device structures
equal a fresh build's, otherwise they are untouched; one small frame per scene is held against the oracle.  The shapes are chosen
for what they can break: mask words and their edges, rows of 64, 65 and 1, bounds off the word grid, triangles cut into slabs,
holes, shells, whole-row flips, centres on faces, edges and vertices, the modes, the refusals, the limits, the streams."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import brush_common as bc
import stream_common as sc_
import voxelize_common as vc
import voxelize_native as N
import voxelize_reference as R
from helpers import metallic_palette

pytestmark = pytest.mark.gpu

BOTH = pytest.mark.parametrize("bricks", [False, True], ids=["dense", "bricks"])
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "voxel-raytracing_amd", "host", "vrt_app")
COVER = {}                                                       # covered() of the reference by case: dense and bricks share it


def dims_of(vol):
    return (vol.shape[2], vol.shape[1], vol.shape[0])


class Scene:
    """a scene of `vol` with textures; voxelize() runs one call on the scene and on the reference and compares everything"""
    def __init__(self, vrt, oracle, engine, vol, bricks, spare=400):
        self.vrt, self.oracle, self.engine, self.vol, self.bricks = vrt, oracle, engine, vol, bricks
        self.pal = metallic_palette(vrt)
        self.sky, self.noise = vrt.synthetic.sky_gradient(64, 32), vrt.synthetic.blue_noise_standin(64)
        self.sc = bc.make_scene(vrt, engine, vol, self.pal, bricks, sky=self.sky, noise=self.noise, spare=spare)

    def voxelize(self, mesh, vid, mode="set", fill="surface", bounds=None, match=0, what="", key=None):
        v, t = mesh
        cover = COVER.setdefault(key, {}) if key is not None else None
        exp_vol, exp = R.voxelize(self.vol, v, t, vid, mode, fill, bounds, match, cover=cover)
        before = bc.snapshot(self.vrt, self.sc, self.bricks) if exp["changed"] == 0 else None
        got = self.sc.voxelize(v, t, vid, mode, fill, bounds, match)
        print(what, vid, mode, fill, bounds, got, "items", self.sc.voxelize_items())
        assert got == exp, (what, got, exp)
        assert (bc.whole(self.sc, dims_of(self.vol)) == exp_vol).all(), what
        if exp["changed"]:
            bc.assert_state_equals_fresh(self.vrt, self.engine, self.sc, exp_vol, self.pal, self.bricks, what)
        else:
            assert bc.same_snapshot(before, bc.snapshot(self.vrt, self.sc, self.bricks)), what
        self.vol = exp_vol
        return exp

    def frame(self, what, planes=bc.GB):
        return bc.assert_frame_equals_oracle(self.vrt, self.oracle, self.engine, self.sc, self.vol, self.pal, self.sky, self.noise, dims_of(self.vol), what, planes)

    def done(self, what):
        self.frame(what)
        self.sc.destroy()


def zeros(dims):
    return np.zeros((dims[2], dims[1], dims[0]), np.uint8)


def tri_mesh(*tris):
    v = np.asarray(tris, np.int32).reshape(-1, 3)
    return v, np.arange(v.shape[0], dtype=np.uint32).reshape(-1, 3)


@BOTH
def test_mask_words_and_rows(vrt, oracle, engine, bricks):
    """triangles inside one mask word and across bits 63 | 64, with the bounds on and off the word grid of the volume, and rows of
    exactly 64, 65 and 1 voxels"""
    dims = (136, 16, 24)
    s = Scene(vrt, oracle, engine, zeros(dims), bricks)
    inside = tri_mesh(((5 * 16 + 3, 20, 30), (20 * 16 + 1, 100, 60), (9 * 16, 200, 200)))
    straddle = tri_mesh(((60 * 16 + 5, 40, 150), (68 * 16 + 2, 90, 170), (63 * 16 + 9, 220, 300)))
    assert s.voxelize(inside, 3, what="inside word 0", key="w-inside")["covered"] > 20
    r = s.voxelize(straddle, 4, what="bits 63 and 64", key="w-straddle")
    assert r["lo"][0] <= 63 and r["lo"][0] + r["size"][0] > 64
    long = tri_mesh(((2 * 16, 10, 20), (130 * 16 + 7, 120, 200), (70 * 16, 250, 380)), ((1, 1, 1), (135 * 16, 255, 383), (135 * 16, 1, 383)))
    for k, (lo_x, size_x) in enumerate(((37, 64), (37, 65), (37, 1), (0, 64), (64, 65), (100, 36), (5, 130), (63, 2))):
        for fill in ("surface", "both"):
            s.voxelize(long, 10 + k, "set", fill, ((lo_x, 0, 0), (size_x, 16, 24)), what=f"row of {size_x} at {lo_x}", key=f"w-long-{k}")
    s.done("mask words")


@BOTH
def test_a_triangle_cut_into_slabs(vrt, oracle, engine, bricks):
    dims = (48, 48, 48)
    s = Scene(vrt, oracle, engine, zeros(dims), bricks)
    big = tri_mesh(((-40, 30, 10), (800, 700, 90), (100, 200, 760)))
    s.voxelize(big, 5, what="default items", key="slab-big")
    one = s.sc.voxelize_items()
    s.sc.voxelize_item_rows(3)
    s.voxelize(big, 6, what="three rows an item", key="slab-big")
    assert s.sc.voxelize_items() > 8 * one
    tet = vc.tetra_mesh(((40, 50, 60), (700, 90, 100), (300, 720, 200), (350, 300, 700)))
    s.sc.voxelize_item_rows(1)
    s.voxelize(tet, 7, "set", "both", what="one row an item, solid", key="slab-tet")
    many = s.sc.voxelize_items()
    s.sc.voxelize_item_rows(0)
    s.voxelize(tet, 8, "set", "both", what="default again", key="slab-tet")
    assert s.sc.voxelize_items() < many
    s.done("slabs")


def solid_cases():
    shell = vc.merge(vc.box_mesh((64, 64, 64), (448, 400, 320)), vc.box_mesh((128, 112, 112), (384, 352, 272), flip=True))
    return [("tetrahedron", vc.tetra_mesh(((35, 50, 60), (600, 90, 100), (300, 620, 200), (350, 300, 330)))),
            ("torus", vc.torus_mesh((24.0, 24.0, 12.0), 14.0, 5.0)),
            ("shell", shell),
            ("sphere", vc.sphere_mesh((20.3, 22.1, 11.7), 9.4)),
            ("aligned box", vc.box_mesh((16, 32, 48), (16 + 64, 32 + 80, 48 + 96))),
            ("centres on faces", vc.box_mesh((40, 40, 40), (104, 104, 104))),
            ("centres on edges", vc.tetra_mesh(((40, 40, 40), (40 + 256, 40, 40), (40, 40 + 256, 40), (40, 40, 40 + 256)))),
            ("centres on vertices", vc.tetra_mesh(((72, 72, 72), (72 + 160, 72, 72), (72, 72 + 160, 72), (72, 72, 72 + 160))))]


@BOTH
def test_solid_shapes(vrt, oracle, engine, bricks):
    dims = (48, 48, 24)
    s = Scene(vrt, oracle, engine, zeros(dims), bricks)
    counts = {}
    for k, (name, mesh) in enumerate(solid_cases()):
        s.voxelize(mesh, 0, "set", "both", ((0, 0, 0), dims), what="clear", key=f"solid-{name}-both")
        counts[name] = s.voxelize(mesh, 20 + k, "set", "solid", ((0, 0, 0), dims), what=name, key=f"solid-{name}")["covered"]
        s.voxelize(mesh, 40 + k, "add", "both", what=name + " with its surface", key=f"solid-{name}-own")
    assert counts["aligned box"] == 4 * 5 * 6 and counts["centres on faces"] == 64
    assert counts["shell"] == 24 * 21 * 16 - 16 * 15 * 10
    s.done("solids")


@BOTH
def test_whole_row_flip_and_parts(vrt, oracle, engine, bricks):
    """a closed mesh partly outside the volume and partly outside the bounds on the +x side: crossings beyond the rows' end flip
    whole rows; and a solid voxelized in parts equals the solid voxelized in one piece"""
    dims = (48, 24, 24)
    mesh = vc.merge(vc.box_mesh((10 * 16, 40, 56), (90 * 16 + 8, 300, 280)), vc.tetra_mesh(((-200, 100, 100), (1200, 150, 120), (300, 370, 200), (350, 200, 390))))
    s = Scene(vrt, oracle, engine, zeros(dims), bricks)
    r = s.voxelize(mesh, 9, "set", "solid", ((8, 0, 0), (22, 24, 24)), what="bounds end inside the mesh", key="flip-a")
    assert r["covered"] > 1500
    whole = Scene(vrt, oracle, engine, zeros(dims), bricks)
    whole.voxelize(mesh, 9, "set", "both", ((0, 0, 0), dims), what="in one piece", key="flip-whole")
    parts = Scene(vrt, oracle, engine, zeros(dims), bricks)
    for k, (lo, size) in enumerate((((0, 0, 0), (17, 24, 11)), ((17, 0, 0), (31, 24, 11)), ((0, 0, 11), (48, 5, 13)), ((0, 5, 11), (48, 19, 13)))):
        parts.voxelize(mesh, 9, "set", "both", (lo, size), what=f"part {k}", key=f"flip-part-{k}")
    assert (parts.vol == whole.vol).all() and (bc.whole(parts.sc, dims) == bc.whole(whole.sc, dims)).all()
    s.done("flip")
    whole.sc.destroy()
    parts.done("parts")


@BOTH
def test_modes_and_noops(vrt, oracle, engine, bricks):
    dims = bc.BRICKS if bricks else bc.DENSE_A
    W, H, D = dims
    vol = bc.brick_volume(dims, 7) if bricks else bc.dense_volume(dims, 11)
    s = Scene(vrt, oracle, engine, vol, bricks)
    ball = vc.sphere_mesh((W / 2.0, H / 2.0, D / 2.0), 13.3)
    slab = vc.box_mesh((16 * 10, 16 * 12 + 3, 16 * 20), (16 * 60 + 5, 16 * 22, 16 * 30 + 9))     # crosses the block of BLOCK_ID
    name = "bricks" if bricks else "dense"
    assert s.voxelize(slab, 24, "replace", "both", match=bc.BLOCK_ID, what="replace the block", key=name + "-slab")["changed"] > 50
    assert s.voxelize(ball, 22, "paint", "both", what="paint", key=name + "-ball")["changed"] > 0
    assert s.voxelize(ball, 23, "add", "both", what="add", key=name + "-ball")["changed"] > 1000
    assert s.voxelize(ball, 21, "set", "surface", what="set", key=name + "-ball")["changed"] > 500
    # no-ops of each kind: nothing is written, the structures are untouched (voxelize() compares the snapshot)
    for mode, vid, match, what in (("set", 21, 0, "set the id already there"), ("add", 25, 0, "add into what is full"), ("replace", 26, bc.ABSENT_ID, "replace an absent id")):
        r = s.voxelize(ball, vid, mode, "surface", match=match, what="no-op: " + what, key=name + "-ball")
        assert r["changed"] == 0 and r["covered"] > 500
    s.voxelize(ball, 0, "set", "both", what="carve", key=name + "-ball")
    assert s.voxelize(ball, 27, "paint", "solid", what="no-op: paint over air", key=name + "-ball")["changed"] == 0
    assert s.sc.voxelize(ball[0], ball[1], 28, bounds=((W, 0, 0), (5, 5, 5))) == R.ZERO                  # bounds wholly outside the volume
    assert s.sc.voxelize(ball[0], ball[1], 28, bounds=((-9, -9, -9), (9, 9, 9))) == R.ZERO
    assert s.voxelize(ball, 28, "set", "both", ((0, 0, 0), (4, 4, 4)), what="no-op: the mesh outside the bounds", key=name + "-corner")["covered"] == 0
    s.done("modes")


@BOTH
def test_a_voxelized_mirror_makes_rays_bounce(vrt, oracle, engine, bricks):
    dims = bc.BRICKS if bricks else bc.DENSE_A
    W, H, D = dims
    vol = bc.brick_volume(dims, 3) if bricks else bc.dense_volume(dims, 3)
    s = Scene(vrt, oracle, engine, vol, bricks)
    names = bc.GB + ["hit_id", "rays_total"]
    s.frame("before", names)
    wall = vc.box_mesh((-16, -16, 0), (16 * W + 16, 16 * H + 16, 24))               # a wall facing the camera
    assert s.voxelize(wall, bc.METAL_ID, "set", "both", what="metal")["covered"] == 2 * W * H
    exp = s.frame("after", names)
    assert (exp["hit_id"] == bc.METAL_ID).any() and int(exp["rays_total"].max()) > 6
    s.sc.destroy()


def test_bricks_before_reserve_and_with_too_few_slots(vrt, oracle, engine):
    dims = bc.BRICKS
    vol = zeros(dims)
    vol[48:56, 40:48, 0:16] = 9                                              # two whole bricks the mesh does not reach
    pal = metallic_palette(vrt)
    mesh = vc.box_mesh((100, 100, 100), (900, 600, 700))
    raw = bc.make_scene(vrt, engine, vol, pal, True, spare=None)
    snap = bc.snapshot(vrt, raw, True)
    with pytest.raises(vrt._capi.VrtError) as err:
        raw.voxelize(mesh[0], mesh[1], 3, fill="solid")
    assert err.value.code == 7 and "vrt_scene_reserve_bricks" in str(err.value) and bc.same_snapshot(snap, bc.snapshot(vrt, raw, True))
    raw.destroy()
    after, _ = R.voxelize(vol, mesh[0], mesh[1], 3, fill="solid")
    need = int((~bc.brick_occupancy(vol) & bc.brick_occupancy(after)).sum())
    assert need > 20
    s = Scene(vrt, oracle, engine, vol, True, spare=need - 1)
    snap = bc.snapshot(vrt, s.sc, True)
    with pytest.raises(vrt._capi.VrtError) as err:
        s.sc.voxelize(mesh[0], mesh[1], 3, fill="solid")
    assert err.value.code == 7 and bc.same_snapshot(snap, bc.snapshot(vrt, s.sc, True)) and (bc.whole(s.sc, dims) == vol).all()
    s.voxelize(vc.box_mesh((0, 40 * 16, 48 * 16), (16 * 16, 48 * 16, 56 * 16)), 0, "set", "solid", what="delete two bricks: their slots are free again")
    s.voxelize(mesh, 3, "set", "solid", what="now it fits")
    s.done("bricks")


@BOTH
def test_side_limit_512(vrt, engine, bricks):
    dims = (520, 8, 8)
    vol = zeros(dims)
    pal = metallic_palette(vrt)
    sc = bc.make_scene(vrt, engine, vol, pal, bricks, spare=200)
    mesh = vc.merge(tri_mesh(((0, 5, 5), (520 * 16, 100, 120), (260 * 16, 120, 20))), vc.box_mesh((3 * 16 + 8, 24, 24), (600 * 16, 104, 104)))
    bounds = ((4, 0, 0), (512, 8, 8))
    exp_vol, exp = R.voxelize(vol, mesh[0], mesh[1], 6, "set", "both", bounds, cover=COVER.setdefault("side-512", {}))
    got = sc.voxelize(mesh[0], mesh[1], 6, "set", "both", bounds)
    assert got == exp and exp["size"][0] == 512, (got, exp)
    assert (bc.whole(sc, dims) == exp_vol).all()
    bc.assert_state_equals_fresh(vrt, engine, sc, exp_vol, pal, bricks, "512 x 8 x 8")
    with pytest.raises(vrt._capi.VrtError) as err:
        sc.voxelize(mesh[0], mesh[1], 7, bounds=((4, 0, 0), (513, 8, 8)))
    assert err.value.code == 1 and "voxelize in parts" in str(err.value)
    with pytest.raises(vrt._capi.VrtError):
        sc.voxelize(mesh[0], mesh[1], 7)                                     # the mesh's own bounds are 520 long inside the volume
    assert sc.voxelize(mesh[0], mesh[1], 6, "set", "both", ((-7, 0, 0), (519, 8, 8)))["changed"] > 0      # 512 after the clip
    sc.destroy()


@BOTH
def test_65536_tiny_triangles(vrt, oracle, engine, bricks):
    dims = (40, 40, 40)
    s = Scene(vrt, oracle, engine, zeros(dims), bricks, spare=200)
    mesh = vc.tiny_triangles(1 << 16, dims, 3)
    r = s.voxelize(mesh, 12, "set", "surface", ((0, 0, 0), dims), what="2^16 triangles", key="tiny")
    assert r["covered"] > 40000 and 65000 < s.sc.voxelize_items() <= 1 << 16      # (a few lie wholly outside the volume)
    s.done("tiny")


@BOTH
def test_vertices_at_the_range_edges(vrt, oracle, engine, bricks):
    dims = (32, 32, 32)
    s = Scene(vrt, oracle, engine, zeros(dims), bricks, spare=100)
    for k, case in enumerate(N.EDGE_CASES):
        mesh = tri_mesh(np.asarray(case).reshape(3, 3))
        s.voxelize(mesh, 30 + k, "set", "both", ((0, 0, 0), dims), what=f"edge case {k}", key=f"edge-{k}")
    s.done("edges")


def test_errors(vrt, engine):
    K, l = vrt._capi, vrt.lib()
    pal = metallic_palette(vrt)
    vol = bc.dense_volume((32, 24, 16), 2)
    sc = vrt.VoxelScene.from_dense(engine, vol, pal)
    good_v = np.asarray([(10, 10, 10), (200, 40, 30), (50, 220, 100)], np.int32)
    good_t = np.asarray([(0, 1, 2)], np.uint32)

    def rc_of(v=good_v, t=good_t, nv=None, nt=None, mode=0, fill=1, vid=1, match=0, size=(20, 20, 16), j=True, r=True, scene=True, vp=True, tp=True):
        v, t = np.ascontiguousarray(v, np.int32), np.ascontiguousarray(t, np.uint32)
        job = K.Voxelize(mode=mode, fill=fill, id=vid, match=match)
        job.lo[:], job.size[:] = (0, 0, 0), size
        res = K.VoxelizeResult()
        rc = l.vrt_scene_voxelize(engine.ctx, sc.handle if scene else None, v.ctypes.data if vp else None, len(v) if nv is None else nv,
                                  t.ctypes.data if tp else None, len(t) if nt is None else nt, C.byref(job) if j else None, C.byref(res) if r else None)
        return rc, l.vrt_last_error().decode()
    assert rc_of()[0] == 0
    vol, _ = R.voxelize(vol, good_v, good_t, 1, bounds=((0, 0, 0), (20, 20, 16)))
    far = good_v.copy(); far[1, 2] = 131073
    low = good_v.copy(); low[2, 0] = -65537
    for kw in ({"nv": 0}, {"nt": 0}, {"nt": (1 << 20) + 1}, {"nv": (1 << 24) + 1}, {"t": [(0, 1, 3)]}, {"t": [(0, 1, 2), (2, 1, 0xFFFFFFFF)]}, {"v": far}, {"v": low},
               {"mode": 4}, {"mode": -1}, {"fill": 0}, {"fill": 4}, {"fill": 7}, {"mode": 1, "vid": 0}, {"mode": 2, "vid": 0}, {"mode": 3, "vid": 5, "match": 5},
               {"size": (0, 4, 4)}, {"size": (4, 4, (1 << 30) + 1)}, {"j": False}, {"r": False}, {"scene": False}, {"vp": False}, {"tp": False}):
        rc, msg = rc_of(**kw)
        assert rc == 1 and "vrt_scene_voxelize" in msg, (kw, rc, msg)
    assert (bc.whole(sc, (32, 24, 16)) == vol).all()
    with pytest.raises(ValueError):
        sc.voxelize(good_v, good_t, 256)
    sc.destroy()


def test_memory_trim_and_the_count_planes(vrt, engine):
    dims = bc.DENSE_A
    W, H, D = dims
    vol = bc.dense_volume(dims, 5)
    pal = metallic_palette(vrt)
    sc = vrt.VoxelScene.from_dense(engine, vol, pal)
    mesh = vc.sphere_mesh((30.0, 20.0, 25.0), 9.0)
    bare = sc.memory_bytes()
    assert sc.voxelize(mesh[0], mesh[1], 10, fill="both", bounds=((0, 0, 0), dims))["changed"] > 0
    base = sc.memory_bytes()
    rows = H * D
    assert base >= bare + rows * 8 * (2 + 2)                                  # the coverage and the toggle mask are counted
    st, push = bc.frame_setup(vrt, dims)
    vrt.GeometryStage(engine, st, sc, debug_planes=True).record(push); engine.synchronize()      # count planes: the second set of fields
    held = sc.memory_bytes()
    assert held > base + W * H * D * 8
    snap = bc.snapshot(vrt, sc, False)
    got = sc.voxelize(mesh[0], mesh[1], 10, fill="both")                      # a no-op keeps them
    assert got["changed"] == 0 and got["covered"] > 1000 and sc.memory_bytes() == held and bc.same_snapshot(snap, bc.snapshot(vrt, sc, False))
    assert sc.voxelize(mesh[0], mesh[1], 11, fill="both")["changed"] > 0      # a call that writes drops them, as an edit does
    assert sc.memory_bytes() < held
    sc.trim()                                                                # ... and trim drops the masks
    assert sc.memory_bytes() < base
    assert sc.voxelize(mesh[0], mesh[1], 11, fill="both")["changed"] == 0     # and the next call takes them again
    sc.destroy()


@pytest.mark.parametrize("kind", sc_.KINDS)
def test_streams_behind_a_busy_device(vrt, kind):
    """an edit, then a voxelization that must see it (PAINT), then a read, on the HIP null stream, the context's own stream and a
    side stream of the caller, enqueued behind a stall with no synchronise by the caller in between; one synchronise at the end"""
    import torch
    dims = (40, 24, 32)
    vol = zeros(dims)
    pal = metallic_palette(vrt)
    mesh = vc.box_mesh((16 * 4 + 8, 40, 40), (16 * 36, 300, 400))
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
        scene.fill((5, 5, 5), (30, 3, 3), 44)                             # the edit the voxelization must see
        got1 = scene.voxelize(mesh[0], mesh[1], 45, "paint", "solid")
        got2 = scene.voxelize(mesh[0], mesh[1], 46, "add", "both")
        read = scene.read((0, 0, 0), dims)
        engine.synchronize()
        if kind == "own":
            torch.cuda.synchronize()
            lib.vrt_device_free(engine.ctx, stall_p)
        v0 = vol.copy()
        v0[5:8, 5:8, 5:35] = 44
        cover = COVER.setdefault("streams", {})
        v1, r1 = R.voxelize(v0, mesh[0], mesh[1], 45, "paint", "solid", cover=cover)
        v2, r2 = R.voxelize(v1, mesh[0], mesh[1], 46, "add", "both", cover=cover)
        assert r1["changed"] == 270 and got1 == r1, kind
        assert got2 == r2 and (read == v2).all(), kind
        scene.destroy(); engine.destroy()


def test_app_voxelize(vrt, tmp_path):
    """vrt_app --voxelize FILE.obj:ID[:FILL[:MODE]] on a generated OBJ (quads, relative indices, slashes), against the Python
    reader plus the reference"""
    assert os.path.exists(APP), "build with __graft_entry__.build()"
    path = os.path.join(ROOT, "tests", "golden", "vox_multi.vox")
    vol = vrt.vox_flatten_host(open(path, "rb").read())[0].copy()
    D, H, W = vol.shape
    x1, y1, z1 = W * 0.75 + 0.3, H * 0.6 + 0.11, D * 0.5 + 0.27
    verts = [(1.25, 1.5, 0.7), (x1, 1.5, 0.7), (x1, y1, 0.7), (1.25, y1, 0.7), (1.25, 1.5, z1), (x1, 1.5, z1), (x1, y1, z1), (1.25, y1, z1)]
    quads = [(0, 3, 2, 1), (4, 5, 6, 7), (0, 1, 5, 4), (2, 3, 7, 6), (1, 2, 6, 5), (0, 4, 7, 3)]
    outs = []
    for k, (relative, slashes, spec, fill, mode) in enumerate(((False, False, "9", "surface", "set"), (True, True, "11:both:add", "both", "add"))):
        obj, out = tmp_path / f"box{k}.obj", tmp_path / f"out{k}.vox"
        vc.write_obj(str(obj), verts, quads, relative, slashes)
        p = subprocess.run([APP, "--vox", path, "--voxelize", f"{obj}:{spec}", "--save-vox", str(out)], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr
        v, t = vrt.read_obj(str(obj))
        assert v.shape == (8, 3) and t.shape == (12, 3) and (v == vrt.mesh_units(verts)).all()
        exp_vol, exp = R.voxelize(vol, v, t, int(spec.split(":")[0]), mode, fill)
        assert f"voxelize: {exp['covered']} voxels covered, {exp['changed']} changed" in p.stdout, p.stdout
        got = vrt.vox_flatten_host(out.read_bytes())[0]
        assert exp["changed"] > 0 and got.shape == exp_vol.shape and (got == exp_vol).all()
        outs.append(exp_vol)
    assert not (outs[0] == outs[1]).all()
