"""vrt_scene_components, vrt_scene_component_labels and vrt_scene_filter_components on the GPU, held bit for bit to a plain
breadth-first search (tests/components_reference.py): records, result and the full label box of every single-purpose scene of
tests/components_common.py on dense and brick scenes, twice for identical bytes; agreement with vrt_scene_flood, the other device
implementation of connectivity; the filter (despeckle, fill_cavities, keep_largest) against the reference, fresh builds and the
oracle; and the API's rules (bricks and their slots, metal, side limits, stale labels, streams)."""
import ctypes as C

import numpy as np
import pytest

import brush_common as bc
import components_common as cc
import components_reference as R
import flood_common as fc
import stream_common as sc_
from helpers import metallic_palette

pytestmark = pytest.mark.gpu

BOTH = pytest.mark.parametrize("bricks", [False, True], ids=["dense", "bricks"])
NAMES = {R.SOLID: "solid", R.SAME: "same", R.EMPTY: "empty"}


def dims_of(vol):
    return (vol.shape[2], vol.shape[1], vol.shape[0])


def label(sc, match, conn, bounds, cl):
    """one labelling -> (records, result, the label box of the clipped bounds or None)"""
    rec, res = sc.components(NAMES[match], conn, bounds)
    return rec, res, sc.labels(cl) if cl is not None else None


@BOTH
@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_labelling_equals_the_reference(vrt, engine, name, bricks):
    vol = cc.volume(name)
    pal = metallic_palette(vrt)
    # the brick scenes of every other case were never reserved: labelling reads, it does not edit
    sc = bc.make_scene(vrt, engine, vol, pal, bricks, spare=None if len(name) % 2 else bc.BRICK_SPARE)
    snap = bc.snapshot(vrt, sc, bricks)
    for k, (match, conn, bounds) in enumerate(cc.CASES[name][1]):
        exp = cc.answer(name, match, conn, bounds)
        rec, res, labels = label(sc, match, conn, bounds, exp[3])
        print(name, NAMES[match], conn, bounds, res)
        cc.assert_same(rec, res, labels, exp, (name, match, conn, bounds))
        if k == 0:                                                # the same labelling again: identical bytes
            rec2, res2, labels2 = label(sc, match, conn, bounds, exp[3])
            assert res2 == res and rec2.tobytes() == rec.tobytes() and labels2.tobytes() == labels.tobytes()
    assert bc.same_snapshot(snap, bc.snapshot(vrt, sc, bricks)) and (bc.whole(sc, dims_of(vol)) == vol).all()
    sc.destroy()


@BOTH
def test_agrees_with_flood(vrt, engine, bricks):
    """two device implementations of connectivity: for the first few and the largest component, a measuring flood from the root
    reports the record's count and box"""
    name = "random_0.31_1"
    vol = cc.volume(name)
    sc = bc.make_scene(vrt, engine, vol, metallic_palette(vrt), bricks, spare=None)
    for match, conn, bounds in ((R.SOLID, 6, None), (R.SAME, 26, None), (R.EMPTY, 6, None), (R.SOLID, 26, ((3, 5, 1), (30, 19, 21)))):
        rec, res = sc.components(NAMES[match], conn, bounds)
        assert res["components"] > 1
        for k in sorted({0, 1, 2, 3, res["largest"]} & set(range(res["components"]))):
            got = sc.region(tuple(int(v) for v in rec[k]["root"]), "solid" if match == R.SOLID else "same", conn, bounds)
            assert got == (int(rec[k]["voxels"]), tuple(int(v) for v in rec[k]["lo"]), tuple(int(v) for v in rec[k]["size"])), (match, conn, k, got, rec[k])
    sc.destroy()


class Scene:
    """a scene of `vol` with textures; every filter is held to the reference, a fresh build and, when the scene goes, the oracle"""
    def __init__(self, vrt, oracle, engine, vol, bricks, spare=bc.BRICK_SPARE):
        self.vrt, self.oracle, self.engine, self.vol, self.bricks = vrt, oracle, engine, vol, bricks
        self.pal = metallic_palette(vrt)
        self.sky, self.noise = vrt.synthetic.sky_gradient(64, 32), vrt.synthetic.blue_noise_standin(64)
        self.sc = bc.make_scene(vrt, engine, vol, self.pal, bricks, sky=self.sky, noise=self.noise, spare=spare)

    def filter(self, what, vid, match="solid", conn=6, **kw):
        exp_vol, exp = R.filter_components(self.vol, vid, match, conn, **kw)
        before = bc.snapshot(self.vrt, self.sc, self.bricks) if exp["changed"] == 0 else None
        got = self.sc.filter_components(vid, match, conn, **kw)
        print(what, vid, match, conn, kw, got)
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


def noised_solid():
    """32^3: an ellipsoid (what a voxelization leaves) and seeded specks of one to a few voxels around it"""
    z, y, x = np.indices((32, 32, 32))
    vol = (((x - 15.5) / 9.0) ** 2 + ((y - 15.5) / 7.0) ** 2 + ((z - 15.5) / 11.0) ** 2 <= 1.0).astype(np.uint8) * 12
    rng = np.random.default_rng(3)
    specks = (rng.random(vol.shape) < 0.06) & (vol == 0)
    vol[specks] = 4
    return vol


@BOTH
def test_despeckle_and_keep_largest(vrt, oracle, engine, bricks):
    s = Scene(vrt, oracle, engine, noised_solid(), bricks)
    res = s.filter("measure", 0, max_voxels=2, measure=True)
    assert res["components"] > 50 and res["changed"] == 0
    assert s.filter("nothing selected", 0, min_voxels=10 ** 6)["components"] == 0
    assert s.filter("under 26 more hangs together: the lone voxels", 0, conn=26, max_voxels=1)["changed"] > 0
    exp_vol, exp = R.filter_components(s.vol, 0, max_voxels=2)
    assert exp["changed"] > 0 and s.sc.despeckle(3) == exp                                     # the one-liner is that filter
    s.vol = exp_vol
    assert (bc.whole(s.sc, dims_of(s.vol)) == s.vol).all()
    bc.assert_state_equals_fresh(vrt, engine, s.sc, s.vol, s.pal, bricks, "despeckle")
    left = s.sc.components()[1]["components"]
    assert left > 1
    exp_vol, exp = R.filter_components(s.vol, 0, keep_largest=True)
    assert s.sc.keep_largest() == exp and exp["components"] == left - 1
    s.vol = exp_vol
    assert (bc.whole(s.sc, dims_of(s.vol)) == s.vol).all() and s.sc.components()[1]["components"] == 1
    bc.assert_state_equals_fresh(vrt, engine, s.sc, s.vol, s.pal, bricks, "keep_largest")
    assert s.filter("again: nothing to do", 0, keep_largest=True)["changed"] == 0
    s.done("despeckle")


@BOTH
def test_fill_cavities(vrt, oracle, engine, bricks):
    s = Scene(vrt, oracle, engine, cc.volume("cavities").copy(), bricks)
    exp_vol, exp = R.filter_components(s.vol, 30, "empty", 6, faces_none=63)
    assert exp["components"] == 1 and exp["changed"] == 6 * 8 * 4                             # the closed one; the leaking one is outer air
    assert s.sc.fill_cavities(30) == exp
    s.vol = exp_vol
    assert (bc.whole(s.sc, dims_of(s.vol)) == s.vol).all()
    bc.assert_state_equals_fresh(vrt, engine, s.sc, s.vol, s.pal, bricks, "fill_cavities")
    assert s.filter("EMPTY with id 0 changes nothing", 0, "empty", 6)["changed"] == 0
    assert s.filter("SAME with the id already there", 8, "same", 6, min_voxels=100, faces_none=63, bounds=((0, 0, 0), (30, 24, 32)))["changed"] == 0
    assert s.filter("recolour what touches -x of off-grid bounds", 77, "same", 26, bounds=((9, 3, 5), (25, 40, 20)), faces_all=1)["changed"] > 0
    s.done("cavities")


def test_api_rules_on_bricks(vrt, oracle, engine):
    dims = bc.BRICKS
    vol = np.zeros((dims[2], dims[1], dims[0]), np.uint8)
    vol[4:44, 4:44, 4:60] = 8; vol[5:43, 5:43, 5:59] = 0                    # a closed shell around 6 x 4 x 4 whole bricks of air
    vol[48:56, 0:8, 0:16] = 9                                                # an object of two whole bricks
    pal = metallic_palette(vrt)
    sc = bc.make_scene(vrt, engine, vol, pal, True, spare=None)            # never reserved
    snap = bc.snapshot(vrt, sc, True)
    assert sc.filter_components(0, measure=True)["components"] == 2 and sc.components("empty")[1]["components"] == 2
    with pytest.raises(vrt._capi.VrtError) as err:
        sc.keep_largest()
    assert err.value.code == 7 and "vrt_scene_reserve_bricks" in str(err.value)
    assert bc.same_snapshot(snap, bc.snapshot(vrt, sc, True))
    sc.destroy()
    filled = vol.copy()
    filled[5:43, 5:43, 5:59] = 12
    need = int((~bc.brick_occupancy(vol) & bc.brick_occupancy(filled)).sum())
    assert need >= 10
    s = Scene(vrt, oracle, engine, vol, True, spare=need - 1)
    snap = bc.snapshot(vrt, s.sc, True)
    with pytest.raises(vrt._capi.VrtError) as err:
        s.sc.fill_cavities(12)
    assert err.value.code == 7 and "vrt_scene_reserve_bricks" in str(err.value)
    assert bc.same_snapshot(snap, bc.snapshot(vrt, s.sc, True)) and (bc.whole(s.sc, dims) == vol).all()       # byte for byte as before
    assert s.filter("delete the smaller object: two bricks free their slots", 0, keep_largest=True)["changed"] == 1024
    assert s.filter("the cavity fill takes free slots", 12, "empty", 6, faces_none=63)["voxels"] == 38 * 38 * 54
    s.done("bricks")


@BOTH
def test_metal_written_by_a_filter_is_seen(vrt, oracle, engine, bricks):
    dims = bc.BRICKS if bricks else bc.DENSE_A
    W, H, D = dims
    vol = bc.brick_volume(dims, 3) if bricks else bc.dense_volume(dims, 3)
    vol[0:2, :, :] = bc.ABSENT_ID                                                      # a wall facing the camera
    s = Scene(vrt, oracle, engine, vol, bricks)
    names = bc.GB + ["hit_id", "rays_total"]
    s.frame("before", names)
    assert s.filter("metal", bc.METAL_ID, "same", 6, min_voxels=2 * W * H, faces_all=0b011111)["changed"] == 2 * W * H
    exp = s.frame("after", names)
    assert (exp["hit_id"] == bc.METAL_ID).any() and int(exp["rays_total"].max()) > 6          # the mirror is seen, and bounces
    s.sc.destroy()


def test_side_limit_512(vrt, engine):
    vol = np.zeros((8, 8, 520), np.uint8)                                    # one thin slab, not a cube
    vol[4, 3, :] = 5; vol[2, 2:6, 100:300:7] = 6; vol[6, 6, 515:] = 7
    sc = vrt.VoxelScene.from_dense(engine, vol, metallic_palette(vrt))
    for match, conn, bounds in ((R.SOLID, 6, ((4, 0, 0), (512, 8, 8))), (R.SAME, 26, ((-7, 0, 0), (519, 8, 8))), (R.EMPTY, 6, ((8, 0, 0), (512, 8, 8)))):
        records, result, labels, cl = R.components(vol, match, conn, bounds)
        assert cl[1] == (512, 8, 8)
        rec, res, lab = label(sc, match, conn, bounds, cl)
        cc.assert_same(rec, res, lab, (R.records_array(records, cc.DTYPE), result, labels, cl), (match, conn, bounds))
    assert int(rec[0]["size"][0]) == 512                                       # end to end: tile coordinate 63
    for call in (lambda: sc.components("solid", 6, ((4, 0, 0), (513, 8, 8))), lambda: sc.components(), lambda: sc.despeckle(2),
                 lambda: sc.filter_components(0, measure=True, bounds=((0, 0, 0), (513, 1, 1)))):
        with pytest.raises(vrt._capi.VrtError) as err:
            call()
        assert err.value.code == 1 and "work in parts" in str(err.value)
    assert (bc.whole(sc, dims_of(vol)) == vol).all()
    sc.destroy()


def test_labels_go_stale_and_memory_is_counted(vrt, engine):
    dims = (40, 24, 32)
    vol = fc.random_volume(dims, 0.3, 8)
    pal = metallic_palette(vrt)
    sc = vrt.VoxelScene.from_dense(engine, vol, pal)
    base = sc.memory_bytes()

    def stale(what):
        with pytest.raises(vrt._capi.VrtError) as err:
            sc.labels()
        assert err.value.code == 1 and what in str(err.value), str(err.value)
    stale("no labelling")
    bounds = ((2, 3, 4), (30, 20, 20))
    _, _, exp_labels, cl = R.components(vol, R.SOLID, 6, bounds)
    sc.components("solid", 6, bounds)
    assert sc.memory_bytes() >= base + 30 * 20 * 20 * 4                       # the label volume is counted
    assert (sc.labels(cl) == exp_labels).all()
    assert (sc.labels(((5, 6, 7), (11, 3, 9))) == exp_labels[3:12, 3:6, 3:14]).all()      # a box inside the bounds
    for box in (((1, 3, 4), (4, 4, 4)), ((2, 3, 4), (31, 20, 20)), ((0, 0, 0), dims)):
        with pytest.raises(vrt._capi.VrtError) as err:
            sc.labels(box)
        assert err.value.code == 1 and "leaves the bounds" in str(err.value)
    assert sc.flood((0, 0, 0), int(vol[0, 0, 0])) ["changed"] == 0 and sc.region((5, 5, 5))[0] >= 1      # calls that write nothing keep it
    assert (sc.labels(cl) == exp_labels).all()
    edits = [lambda: sc.fill((0, 0, 0), (1, 1, 1), 9), lambda: sc.edit((1, 1, 1), np.full((2, 2, 2), 3, np.uint8)), lambda: sc.box((3, 3, 3), (2, 2, 2), 4),
             lambda: sc.stamp((20, 10, 10), sc, (0, 0, 0), (4, 4, 4)), lambda: sc.flood((1, 1, 1), 17), lambda: sc.dilate(1, 5, bounds=((8, 8, 8), (4, 4, 4))),
             lambda: sc.voxelize(vrt.mesh_units([[1, 1, 1], [9, 1, 1], [1, 9, 1]]), [[0, 1, 2]], 21), lambda: sc.filter_components(0, max_voxels=1)]
    for k, edit in enumerate(edits):
        edit()
        stale("edited after its latest labelling")
        sc.components("solid", 6, bounds)
        sc.labels(cl)
    assert sc.filter_components(0, measure=True)["components"] > 0           # a measuring filter labels too
    sc.labels()
    sc.trim()
    assert sc.memory_bytes() <= base
    stale("no labelling")
    sc.destroy()


def test_errors(vrt, engine):
    K, l = vrt._capi, vrt.lib()
    pal = metallic_palette(vrt)
    vol = bc.dense_volume((32, 24, 16), 2)
    sc = vrt.VoxelScene.from_dense(engine, vol, pal)

    def rc_of(match=0, conn=6, flags=0, size=(4, 4, 4), lo=(0, 0, 0), q=True, r=True, scene=True, filt=None):
        c = K.Components(match=match, connectivity=conn, flags=flags)
        c.lo[:], c.size[:] = lo, size
        if filt is None:
            res = K.ComponentsResult(components=77)
            rc = l.vrt_scene_components(engine.ctx, sc.handle if scene else None, C.byref(c) if q else None, None, 0, C.byref(res) if r else None)
            return rc, l.vrt_last_error().decode(), int(res.components)
        f = K.ComponentFilter(**filt) if filt is not False else None
        res = K.FilterResult()
        rc = l.vrt_scene_filter_components(engine.ctx, sc.handle if scene else None, C.byref(c) if q else None, C.byref(f) if f is not None else None,
                                           C.byref(res) if r else None)
        return rc, l.vrt_last_error().decode(), int(res.components)
    assert rc_of()[0] == 0
    assert rc_of(lo=(100, 0, 0)) == (0, rc_of(lo=(100, 0, 0))[1], 0) and rc_of(lo=(-9, -9, -9), size=(9, 9, 9))[2] == 0       # wholly outside: no components, no error
    for kw in ({"match": 3}, {"match": -1}, {"conn": 18}, {"conn": 0}, {"flags": 1}, {"size": (0, 4, 4)}, {"size": (4, 4, (1 << 30) + 1)}, {"q": False}, {"r": False},
               {"scene": False}):
        rc, msg, _ = rc_of(**kw)
        assert rc == 1 and "vrt_scene_components" in msg, (kw, rc, msg)
        rc, msg, _ = rc_of(filt={"max_voxels": 5}, **kw)
        assert rc == 1 and "vrt_scene_filter_components" in msg, (kw, rc, msg)
    ok = {"min_voxels": 0, "max_voxels": 0, "flags": K.COMP_MEASURE}
    assert rc_of(filt=ok)[0] == 0
    for bad in ({"min_voxels": 2, "max_voxels": 1}, {"max_voxels": 1, "flags": 4}, {"max_voxels": 1, "faces_all": 64}, {"max_voxels": 1, "faces_none": 1 << 31}, False):
        rc, msg, _ = rc_of(filt=bad)
        assert rc == 1 and "vrt_scene_filter_components" in msg, (bad, rc, msg)
    # a short buffer: the count is reported, then VRT_ERR_INVALID, as vrt_scene_list_box
    rec, res = sc.components()
    assert res["components"] > 2
    c = K.Components(match=0, connectivity=6)
    c.lo[:], c.size[:] = (0, 0, 0), (32, 24, 16)
    out, short = K.ComponentsResult(), np.zeros(2, vrt.VoxelScene.COMPONENT_DTYPE)
    assert l.vrt_scene_components(engine.ctx, sc.handle, C.byref(c), short.ctypes.data_as(C.c_void_p), 2, C.byref(out)) == 1
    assert int(out.components) == res["components"] and "room for 2" in l.vrt_last_error().decode() and not short.tobytes().strip(b"\0")
    assert l.vrt_scene_component_labels(engine.ctx, sc.handle, None, None, None) == 1
    assert (bc.whole(sc, (32, 24, 16)) == vol).all()
    with pytest.raises(ValueError):
        sc.filter_components(256)
    sc.destroy()


@pytest.mark.parametrize("kind", sc_.KINDS)
def test_streams_behind_a_busy_device(vrt, kind):
    """an edit, then a labelling that must see it, then a filter, on the HIP null stream, the context's own stream and a side stream of
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
        scene.fill((5, 5, 5), (30, 3, 3), 44)                             # the edit the labelling must see
        rec, res = scene.components("same", 26)
        labels = scene.labels()
        got = scene.despeckle(4, 26)
        read = scene.read((0, 0, 0), dims)
        engine.synchronize()
        if kind == "own":
            torch.cuda.synchronize()
            lib.vrt_device_free(engine.ctx, stall_p)
        v0 = vol.copy()
        v0[5:8, 5:8, 5:35] = 44
        records, result, exp_labels, cl = R.components(v0, R.SAME, 26)
        cc.assert_same(rec, res, labels, (R.records_array(records, cc.DTYPE), result, exp_labels, cl), kind)
        assert int(rec[int(exp_labels[6, 6, 6])]["voxels"]) == 270
        v1, exp = R.filter_components(v0, 0, R.SOLID, 26, max_voxels=3)
        assert got == exp and (read == v1).all(), kind
        scene.destroy(); engine.destroy()


def test_app_components_in_order_then_save(vrt, tmp_path):
    """vrt_app --fill ... --components ... --despeckle N --fill-cavities ID --keep-largest --save-vox OUT (the C++ mirror): one line per
    component, and the saved file loads to the volume the reference composes"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    app = os.path.join(root, "voxel-raytracing_amd", "host", "vrt_app")
    assert os.path.exists(app), "build with __graft_entry__.build()"
    path = os.path.join(root, "tests", "golden", "vox_multi.vox")
    vol = vrt.vox_flatten_host(open(path, "rb").read())[0].copy()
    D, H, W = vol.shape
    out = tmp_path / "filtered.vox"
    args = ["--fill", "0", "0", "0", "1", "1", "1", "7", "--components", "solid:6", "--components", f"same:26:-2,0,0:{W},{H},{D}", "--despeckle", "2",
            "--fill-cavities", "9", "--keep-largest"]
    p = subprocess.run([app, "--vox", path] + args + ["--save-vox", str(out)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    vol[0, 0, 0] = 7
    records, result, _, _ = R.components(vol, R.SOLID, 6)
    assert f"components: {result['components']}, {result['voxels']} voxels, largest {result['largest']}\n" in p.stdout, p.stdout
    for k, r in enumerate(records):
        line = "component %d: root %d %d %d id %d voxels %d box %d %d %d + %d %d %d faces %d\n" % ((k,) + r["root"] + (r["id"], r["voxels"]) + r["lo"] + r["size"] + (r["faces"],))
        assert line in p.stdout, (line, p.stdout)
    result2 = R.components(vol, R.SAME, 26, ((-2, 0, 0), (W, H, D)))[1]
    assert f"components: {result2['components']}, {result2['voxels']} voxels, largest {result2['largest']}\n" in p.stdout, p.stdout
    for what, kw in (("despeckle", dict(vid=0, max_voxels=1)), ("fill-cavities", dict(vid=9, match=R.EMPTY, faces_none=63)), ("keep-largest", dict(vid=0, keep_largest=True))):
        vol, res = R.filter_components(vol, kw.pop("vid"), kw.pop("match", R.SOLID), 6, **kw)
        assert f"{what}: {res['components']} components of {res['voxels']} voxels selected, {res['changed']} changed" in p.stdout, (what, res, p.stdout)
    got = vrt.vox_flatten_host(out.read_bytes())[0]
    assert got.shape == vol.shape and (got == vol).all()
