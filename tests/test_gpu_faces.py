"""vrt_scene_list_faces on the GPU, on dense, reserved-brick and unreserved-brick scenes, held record for record to the definition
in numpy (tests/faces_reference.py): the table of boxes of tests/faces_common.py under the four flag sets, a box extracted in eight
parts, the capacity rule, the refusals, an extraction behind an edit and behind a busy device on the three kinds of stream, and the
closed loop -- faces -> quads -> triangles -> vrt_scene_voxelize(SOLID) into an empty scene gives the occupancy back -- directly and
through an OBJ file, from Python and from vrt_app."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import faces_common as fc
import faces_reference as R
import stream_common as sc_
from helpers import metallic_palette

pytestmark = pytest.mark.gpu

KIND = pytest.mark.parametrize("kind", fc.KINDS)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "voxel-raytracing_amd", "host", "vrt_app")


@pytest.fixture(scope="module")
def scenes(vrt, engine):
    """the scene of a named volume and kind, built once"""
    made = {}

    def get(vol_name, kind):
        if (vol_name, kind) not in made:
            made[(vol_name, kind)] = fc.make_scene(vrt, engine, fc.volume(vol_name), metallic_palette(vrt), kind)
        return made[(vol_name, kind)]
    yield get
    for sc in made.values():
        sc.destroy()


def same(got, want, what):
    (rec, counts), (erec, ecounts) = got, want
    assert counts.tolist() == ecounts.tolist(), (what, counts, ecounts)
    assert rec.shape == erec.shape and (rec == erec).all(), what


@KIND
@pytest.mark.parametrize("case", fc.CASES, ids=[c[0] for c in fc.CASES])
def test_the_table(scenes, kind, case):
    name, vol_name, lo, size = case
    sc = scenes(vol_name, kind)
    for runs, closed in fc.FLAGS:
        want = fc.expected(vol_name, lo, size, runs, closed)
        same(sc.faces(lo, size, runs, closed), want, (name, kind, runs, closed))
        assert sc.face_count(lo, size, runs, closed).tolist() == want[1].tolist()
    print(name, kind, [int(fc.expected(vol_name, lo, size, r, False)[1].sum()) for r in (False, True)])


@KIND
def test_eight_parts_unite_to_the_whole(scenes, kind):
    sc = scenes("random", kind)
    lo, size = fc.RANDOM_BOX
    for runs in (False, True):
        whole = R.unit_faces(sc.faces(lo, size, runs)[0], lo)
        parts = [R.unit_faces(sc.faces(plo, psize, runs)[0], plo) for plo, psize in fc.eight_parts(lo, size)]
        assert (np.sort(np.concatenate(parts)) == whole).all(), (kind, runs)      # (sorted keys: no face twice, none missing)
    assert whole.size == int(fc.expected("random", lo, size, False, False)[1].sum())


@KIND
def test_the_capacity_rule(vrt, engine, scenes, kind):
    sc, lib = scenes("random", kind), vrt.lib()
    lo, size = (9, 7, 5), (40, 20, 10)
    want, wc = fc.expected("random", lo, size, True, False)
    clo, csz = (C.c_int32 * 3)(*lo), (C.c_uint32 * 3)(*size)
    counts = (C.c_uint64 * 6)(*[77] * 6)
    guard = np.full(want.size + 8, 0xA5A5A5A5A5A5A5A5, np.uint64)
    rc = lib.vrt_scene_list_faces(engine.ctx, sc.handle, clo, csz, 1, guard.ctypes.data_as(C.c_void_p), want.size - 1, counts)
    assert rc == 1 and b"room for" in lib.vrt_last_error()
    assert list(counts) == wc.tolist() and (guard == 0xA5A5A5A5A5A5A5A5).all()
    rc = lib.vrt_scene_list_faces(engine.ctx, sc.handle, clo, csz, 1, guard.ctypes.data_as(C.c_void_p), want.size, counts)
    assert rc == 0 and (guard[:want.size] == want).all() and (guard[want.size:] == 0xA5A5A5A5A5A5A5A5).all()


def test_the_refusals(vrt, engine, scenes):
    sc, lib = scenes("long-x", "dense"), vrt.lib()
    rec = np.zeros(16, np.uint64)

    def rc_of(lo=(0, 0, 0), size=(4, 4, 4), flags=0, scene=True, ctx=True, l=True, s=True, c=True):
        counts = (C.c_uint64 * 6)()
        rc = lib.vrt_scene_list_faces(engine.ctx if ctx else None, sc.handle if scene else None, (C.c_int32 * 3)(*lo) if l else None,
                                      (C.c_uint32 * 3)(*size) if s else None, flags, rec.ctypes.data_as(C.c_void_p), 16, counts if c else None)
        return rc, lib.vrt_last_error().decode()
    for kw in ({"size": (257, 4, 4)}, {"size": (0, 4, 4)}, {"size": (4, 4, 0)}, {"lo": (261, 0, 0)}, {"lo": (0, 5, 0)}, {"lo": (-1, 0, 0)}, {"lo": (0, 0, 8)},
               {"flags": 4}, {"flags": 0x80000001}, {"scene": False}, {"ctx": False}, {"l": False}, {"s": False}, {"c": False}):
        rc, msg = rc_of(**kw)
        assert rc == 1 and "vrt_scene_list_faces" in msg, (kw, rc, msg)
    assert (rec == 0).all()
    with pytest.raises(vrt._capi.VrtError) as err:
        vrt._capi.check(lib.vrt_scene_save_obj_file(engine.ctx, sc.handle, b"x.obj", 3))      # RUNS | CLOSED
    assert err.value.code == 1 and "seams" in str(err.value)
    with pytest.raises(RuntimeError, match="Could not write mesh"):          # VRT_ERR_IO
        sc.save_obj("/nonexistent-directory/x.obj")


@pytest.mark.parametrize("kind", ["dense", "reserved"])
def test_faces_behind_a_carve_see_it(vrt, engine, kind):
    vol = fc.volume("random").copy()
    sc = fc.make_scene(vrt, engine, vol, metallic_palette(vrt), kind)
    changed, _, _ = sc.brush("box", "set", (10, 9, 8, 30, 20, 17), 0)
    got = sc.faces(*fc.RANDOM_BOX)                                   # no synchronise by the caller in between
    vol[8:25, 9:29, 10:40] = 0
    assert changed > 4000
    same(got, R.faces(vol, *fc.RANDOM_BOX), kind)
    sc.destroy()


@pytest.mark.parametrize("kind", sc_.KINDS)
def test_streams_behind_a_busy_device(vrt, kind):
    """an edit, then an extraction that must see it, on the HIP null stream, the context's own stream and a side stream of the
    caller, enqueued behind a stall with no synchronise by the caller in between"""
    import torch
    vol = fc.volume("random")
    side = torch.cuda.Stream() if kind == "side" else None
    with torch.cuda.stream(side if side is not None else torch.cuda.default_stream()):
        engine = vrt.Engine(0, use_torch_stream=kind != "own")
        lib, cap = vrt.lib(), vrt._capi
        scene = vrt.VoxelScene.from_dense(engine, vol, metallic_palette(vrt))
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
        scene.fill((5, 5, 5), (30, 3, 3), 0)                              # the edit the extraction must see
        got = scene.faces(*fc.RANDOM_BOX)
        engine.synchronize()
        if kind == "own":
            torch.cuda.synchronize()
            lib.vrt_device_free(engine.ctx, stall_p)
        v = vol.copy()
        v[5:8, 5:8, 5:35] = 0
        same(got, R.faces(v, *fc.RANDOM_BOX), kind)
        scene.destroy(); engine.destroy()


LOOP_DIMS = (40, 24, 20)


def loop_volume():
    """a random 40 x 24 x 20 volume under four empty layers: 40 x 24 x 24, a whole number of bricks"""
    return np.pad(fc._random(LOOP_DIMS, 17), ((0, 4), (0, 0), (0, 0)))


@KIND
def test_the_closed_loop_on_the_device(vrt, engine, kind):
    vol = loop_volume()
    pal = metallic_palette(vrt)
    src = fc.make_scene(vrt, engine, vol, pal, kind)
    rec, _ = src.faces((0, 0, 0), LOOP_DIMS, runs=True)
    v, q, ids = vrt.faces_mesh(rec, (0, 0, 0))
    dst = vrt.VoxelScene.from_dense(engine, np.zeros_like(vol), pal)
    r = dst.voxelize(v, vrt.quads_to_triangles(q), 5, fill="solid", bounds=((0, 0, 0), LOOP_DIMS))
    assert r["covered"] == int((vol != 0).sum())
    assert ((dst.read((0, 0, 0), LOOP_DIMS) != 0) == (vol[:LOOP_DIMS[2]] != 0)).all()
    src.destroy(); dst.destroy()


def test_the_closed_loop_through_an_obj_file(vrt, engine, tmp_path):
    vol = loop_volume()
    pal = metallic_palette(vrt)
    src = vrt.VoxelScene.from_dense(engine, vol, pal)
    src.save_obj(str(tmp_path / "loop.obj"))
    obj, mtl = src.to_obj_bytes("loop.mtl")
    assert (tmp_path / "loop.obj").read_bytes() == obj and (tmp_path / "loop.mtl").read_bytes() == mtl
    rec, _ = src.faces((0, 0, 0), LOOP_DIMS)
    assert (obj, mtl) == vrt.faces_obj_host(rec, (0, 0, 0), pal, "loop.mtl")          # one tile: the host-only writer's file
    v, t = vrt.read_obj(str(tmp_path / "loop.obj"))
    dst = vrt.VoxelScene.from_dense(engine, np.zeros_like(vol), pal)
    dst.voxelize(v, t, 5, fill="solid", bounds=((0, 0, 0), LOOP_DIMS))
    assert ((dst.read((0, 0, 0), LOOP_DIMS) != 0) == (vol[:LOOP_DIMS[2]] != 0)).all()
    src.destroy(); dst.destroy()


def test_app_save_obj(vrt, engine, tmp_path):
    """vrt_app --fill ... --save-obj writes the file the Python mirror writes, byte for byte"""
    assert os.path.exists(APP), "build with __graft_entry__.build()"
    path = os.path.join(ROOT, "tests", "golden", "vox_multi.vox")
    vol, pal = vrt.vox_flatten_host(open(path, "rb").read())[:2]
    vol = vol.copy()
    D, H, W = vol.shape
    box = (1, 1, 0, min(5, W - 1), min(4, H - 1), min(3, D))
    (tmp_path / "app").mkdir(); (tmp_path / "py").mkdir()
    p = subprocess.run([APP, "--vox", path, "--fill", *[str(t) for t in box], "9", "--save-obj", str(tmp_path / "app" / "s.obj")],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    vol[box[2]:box[2] + box[5], box[1]:box[1] + box[4], box[0]:box[0] + box[3]] = 9
    sc = vrt.VoxelScene.from_dense(engine, vol, pal)
    sc.save_obj(str(tmp_path / "py" / "s.obj"))
    sc.destroy()
    for name in ("s.obj", "s.mtl"):
        a, b = (tmp_path / "app" / name).read_bytes(), (tmp_path / "py" / name).read_bytes()
        assert len(a) > 100 and a == b, name
