"""vrt_scene_brush and vrt_scene_stamp at their documented limits, on the device: the tables of tests/brush_limits_common.py (which
tests/test_brush_limits_cpu.py proves to reach what they claim) with the checks of test_gpu_brush.py after every operation --
the returned (changed, lo, size) and the whole volume against tests/brush_reference.py (Python integers), a no-op leaves every
structure byte-identical, the structures equal a fresh build's -- and frames against the oracle.  Every comparison is exact.
  A  semi-axes of 1024, capsule ends at -4096 and 12288, boxes of 2^30: the int64 products and the bounds, per lane
  B  4096-long scenes, dense and as 512 bricks: 64 segments per row, a tight box 4096 long, coordinate 4095, brick 511
  C  the ids a stamp writes, which decide whether the scene's rays may bounce
  D  stamps with a side of 512 in every permutation, destinations at the int32 edges, 512 KiB of staging
  E  VoxelScene::brush and VoxelScene::stamp of the C++ mirror (tests/native/brush_limits_main.cpp)"""
import os
import subprocess

import numpy as np
import pytest

import brush_common as bc
import brush_limits_common as L
import brush_reference as R
import extents_common as X
from helpers import compare_planes, metallic_palette
from ray_query_common import oracle_records, planes_differ

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METAL_PLANES = bc.GB + ["hit_id", "rays_total"]


@pytest.fixture(scope="module")
def textures(vrt):
    return metallic_palette(vrt), vrt.synthetic.sky_gradient(64, 32), vrt.synthetic.blue_noise_standin(64)


def tup(res):
    return (res[0], tuple(res[1]), tuple(res[2]))


def run(vrt, sc, bricks, o, res, exp, dims, what, src=None):
    """one brush or stamp, once: the result, a no-op's structures, the whole volume"""
    noop = res[0] == 0
    before = bc.snapshot(vrt, sc, bricks) if noop else None
    if "stamp" in o:
        dlo, slo, size, orient, skip = o["stamp"]
        got = sc.stamp(dlo, sc if src is None else src, slo, size, orient, skip)
    else:
        got = sc.brush(o["shape"], o["mode"], o["p"], o["id"], o["match"])
    assert got == tup(res), (what, got, res)
    if noop:
        assert got == (0, (0, 0, 0), (0, 0, 0)) and bc.same_snapshot(before, bc.snapshot(vrt, sc, bricks)), what
    assert (bc.whole(sc, dims) == exp).all(), what


def makes_or_removes_bricks(before, after):
    return (bc.brick_occupancy(before) != bc.brick_occupancy(after)).any()


# ---- group A ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", L.A_GROUPS)
@pytest.mark.parametrize("name,dims,bricks", L.A_SCENES, ids=[s[0] for s in L.A_SCENES])
def test_shapes_at_their_limits(vrt, engine, textures, name, dims, bricks, group):
    pal = textures[0]
    vol = L.a_volume(dims, bricks)
    sc = bc.make_scene(vrt, engine, vol, pal, bricks, spare=L.all_bricks_spare(vol) if bricks else None)
    try:
        cases = L.group_a(dims)[group]
        for k, (o, (exp, res)) in enumerate(zip(cases, L.a_expected(dims, bricks, group))):
            what = f"{name} {group} ({o['kind']})"
            assert (res[0] == 0) == o["kind"].startswith("no-op"), what
            run(vrt, sc, bricks, o, res, exp, dims, what)
            if k == len(cases) - 1 or (bricks and makes_or_removes_bricks(vol, exp)):
                bc.assert_state_equals_fresh(vrt, engine, sc, exp, pal, bricks, what)
            vol = exp
    finally:
        sc.destroy()


# ---- group B ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,bricks", L.B_SCENES, ids=["%s-%s" % ("bricks" if b else "dense", "x".join(map(str, d))) for d, b in L.B_SCENES])
def test_brushes_on_4096_long_scenes(vrt, oracle, engine, textures, dims, bricks):
    pal, sky, noise = textures
    vol = L.b_volume(dims)
    a = X.long_axis(dims)
    sc = bc.make_scene(vrt, engine, vol, pal, bricks, sky=sky, noise=noise, spare=L.all_bricks_spare(vol) if bricks else None)
    try:
        ops = L.limit_ops(dims)
        for k, (o, (exp, res)) in enumerate(zip(ops, L.b_expected(dims))):
            what = f"{dims} {'bricks' if bricks else 'dense'} ({o['kind']})"
            run(vrt, sc, bricks, o, res, exp, dims, what)
            if o["kind"] == "capsule along the whole axis":
                assert res[2][a] == 4096, what
            if k == len(ops) - 1 or "stamp" in o or (bricks and makes_or_removes_bricks(vol, exp)):
                bc.assert_state_equals_fresh(vrt, engine, sc, exp, pal, bricks, what)
            vol = exp
        # a frame from beyond the far end, looking back along the axis
        res_ = L.B_RES
        _, st = X.render_settings(vrt, res_)[0]
        push = X.push_of(vrt, dims, res_, X.needle_cameras(dims)[0][:4] + (2.0,))
        osn = oracle.OracleScene(vol, pal, sky=sky, noise=noise)
        exp = oracle.render(osn, push, oracle.params_from(st.to_c()), nthreads=8)
        assert (exp["hit_id"] != 0).any()
        g = vrt.GeometryStage(engine, st, sc, debug_planes=True).record(push)
        engine.synchronize()
        bad = compare_planes(g.numpy(), exp, METAL_PLANES)
        assert not bad, (dims, bad[:2])
        # rays along the axis, both ways, against the oracle's single-ray trace
        for sign in (1, -1):
            s, d = X.needle_rays(dims, sign, n=10)
            rec, _ = oracle_records(oracle, osn, s, d, 5000)
            assert (rec["material"] != 0).any()
            bad = planes_differ(sc.trace_rays(s, d, 5000), rec)
            assert bad.size == 0, (dims, sign, bad)
    finally:
        sc.destroy()


# ---- group C ------------------------------------------------------------------------------------------------------------------------
def frame_at(vrt, oracle, engine, sc, vol, pal, sky, noise, dims, position, what):
    """assert_frame_equals_oracle with the camera at `position`, looking along +z: close enough to see one voxel"""
    st, _ = bc.frame_setup(vrt, dims)
    push = vrt.make_push(vrt.CameraController(position=position), dims, bc.RES, frame=2)
    gb = vrt.GeometryStage(engine, st, sc, debug_planes=True).record(push)
    engine.synchronize()
    exp = oracle.render(oracle.OracleScene(vol, pal, sky=sky, noise=noise), push, oracle.params_from(st.to_c()), planes=METAL_PLANES, nthreads=8)
    bad = compare_planes(gb.numpy(), exp, METAL_PLANES)
    assert not bad, (what, bad)
    return exp


def destination(vrt, engine, textures, dims, bricks, pal=None):
    _, sky, noise = textures
    vol = L.a_volume(dims, bricks)
    assert not (vol >= 199).any()
    return vol, bc.make_scene(vrt, engine, vol, pal if pal is not None else textures[0], bricks, sky=sky, noise=noise, spare=L.all_bricks_spare(vol) if bricks else None)


def stamp_checked(vrt, engine, dst, vol, pal, bricks, dims, src, svol, dlo, size, orient, skip, what, slo=(0, 0, 0)):
    exp, res = R.stamp(vol, dlo, svol, slo, size, orient, skip)
    run(vrt, dst, bricks, {"stamp": (dlo, slo, size, orient, skip)}, res, exp, dims, what, src=src)
    bc.assert_state_equals_fresh(vrt, engine, dst, exp, pal, bricks, what)
    return exp, res


@pytest.mark.parametrize("name,dims,bricks", L.A_SCENES, ids=[s[0] for s in L.A_SCENES])
def test_stamp_of_every_id(vrt, oracle, engine, textures, name, dims, bricks):
    pal, sky, noise = textures
    svol = L.all_ids_source()
    vol, dst = destination(vrt, engine, textures, dims, bricks)
    src = vrt.VoxelScene.from_dense(engine, svol, pal)
    try:
        bc.assert_frame_equals_oracle(vrt, oracle, engine, dst, vol, pal, sky, noise, dims, "before", METAL_PLANES)
        size = L.ALL_IDS_DIMS
        vol, res = stamp_checked(vrt, engine, dst, vol, pal, bricks, dims, src, svol, L.face_lo(dims, size), size, 0, False, f"{name} every id")
        assert res[0] >= 250
        exp = bc.assert_frame_equals_oracle(vrt, oracle, engine, dst, vol, pal, sky, noise, dims, f"{name} every id", METAL_PLANES)
        assert (exp["hit_id"] >= 200).any() and int(exp["rays_total"].max()) > 6
        orient = 3 | 5 << 3
        dlo = (5, 7, 0)
        vol, res = stamp_checked(vrt, engine, dst, vol, pal, bricks, dims, src, svol, dlo, size, orient, True, f"{name} every id, turned")
        assert res[0] >= 250
        bc.assert_frame_equals_oracle(vrt, oracle, engine, dst, vol, pal, sky, noise, dims, f"{name} every id, turned", METAL_PLANES)
    finally:
        dst.destroy(); src.destroy()


@pytest.mark.parametrize("vid", L.ONE_ID)
@pytest.mark.parametrize("name,dims,bricks", L.A_SCENES, ids=[s[0] for s in L.A_SCENES])
def test_stamp_of_one_metallic_id_is_seen(vrt, oracle, engine, textures, name, dims, bricks, vid):
    """the stamp form of test_metal_written_by_a_brush_is_seen: the only metallic id the scene ever held comes from the set of
    written ids; were its bit lost, the frame would be rendered without the bounce loop"""
    pal, sky, noise = textures
    svol = L.slab_source(vid)
    vol, dst = destination(vrt, engine, textures, dims, bricks)
    src = vrt.VoxelScene.from_dense(engine, svol, pal)
    try:
        size = L.SLAB_DIMS
        vol, res = stamp_checked(vrt, engine, dst, vol, pal, bricks, dims, src, svol, L.face_lo(dims, size), size, 0, False, f"{name} id {vid}")
        exp = bc.assert_frame_equals_oracle(vrt, oracle, engine, dst, vol, pal, sky, noise, dims, f"{name} id {vid}", METAL_PLANES)
        assert (exp["hit_id"] == vid).any() and int(exp["rays_total"].max()) > 6
    finally:
        dst.destroy(); src.destroy()


@pytest.mark.parametrize("lane_x", [63, 64], ids=["lane-63", "lane-0-of-the-next-segment"])
@pytest.mark.parametrize("name,dims,bricks", L.A_SCENES, ids=[s[0] for s in L.A_SCENES])
def test_stamp_whose_only_metallic_voxel_is_one_lane(vrt, oracle, engine, textures, name, dims, bricks, lane_x):
    pal, sky, noise = textures
    svol = L.one_lane_source(lane_x)
    vol, dst = destination(vrt, engine, textures, dims, bricks)
    src = vrt.VoxelScene.from_dense(engine, svol, pal)
    try:
        size, dlo = (66, 6, 2), (2, dims[1] // 2 - 3, 0)
        vol, res = stamp_checked(vrt, engine, dst, vol, pal, bricks, dims, src, svol, dlo, size, 0, False, f"{name} lane {lane_x}")
        assert res[1][0] == dlo[0] and res[0] > 700                              # the clipped bounds start at dst_lo: lane = source x mod 64
        x, y = dlo[0] + lane_x, dlo[1] + 3
        assert vol[0, y, x] == 255 and int((vol >= 200).sum()) == 1
        exp = frame_at(vrt, oracle, engine, dst, vol, pal, sky, noise, dims, (x + 0.8, y + 0.7, -6.0), f"{name} lane {lane_x}")
        assert (exp["hit_id"] == 255).any() and int(exp["rays_total"].max()) > 6
    finally:
        dst.destroy(); src.destroy()


@pytest.mark.parametrize("name,dims,bricks", L.A_SCENES, ids=[s[0] for s in L.A_SCENES])
def test_stamps_that_bring_no_metal(vrt, oracle, engine, textures, name, dims, bricks):
    """controls: the metallic voxels clipped away, outside the stamped box under SKIP_EMPTY, and a stamp over identical content.
    Whatever they do to the flag, the frame equals the oracle's."""
    pal, sky, noise = textures
    W, H, D = dims
    svol = np.zeros((4, 12, 20), np.uint8)
    svol[:, :, :10] = 255; svol[2:, :, 10:] = L.FILL_ID; svol[:2, :, 10:14] = 230     # metal in x < 10, and before z = 2 in x 10..13
    vol, dst = destination(vrt, engine, textures, dims, bricks)
    src = vrt.VoxelScene.from_dense(engine, svol, pal)
    try:
        frames = lambda what: bc.assert_frame_equals_oracle(vrt, oracle, engine, dst, vol, pal, sky, noise, dims, what, METAL_PLANES)
        vol, res = stamp_checked(vrt, engine, dst, vol, pal, bricks, dims, src, svol, (-10, H // 2 - 6, -2), (20, 12, 4), 0, False, f"{name} clipped away")
        assert res[0] > 0 and not (vol >= 200).any()
        frames("clipped away")
        vol, res = stamp_checked(vrt, engine, dst, vol, pal, bricks, dims, src, svol, (W // 2, 3, 0), (6, 12, 4), 0, True, f"{name} skipped", slo=(14, 0, 0))
        assert res[0] > 0 and not (vol >= 200).any()
        frames("skipped")
        vol, res = stamp_checked(vrt, engine, dst, vol, pal, bricks, dims, src, svol, (W // 2, 3, 0), (6, 12, 4), 0, True, f"{name} identical", slo=(14, 0, 0))
        assert res[0] == 0
        exp = frames("identical")
        assert (exp["hit_id"] == L.FILL_ID).any()
    finally:
        dst.destroy(); src.destroy()


@pytest.mark.parametrize("pair", L.BOUNDARY_PAIRS, ids=lambda p: "%d-%d" % p)
@pytest.mark.parametrize("name,dims,bricks", L.A_SCENES, ids=[s[0] for s in L.A_SCENES])
def test_stamp_of_ids_on_either_side_of_a_word(vrt, oracle, engine, textures, name, dims, bricks, pair):
    """ids 31 / 32, 63 / 64, 223 / 224 under a palette in which they are not metallic and their neighbours in the set are"""
    _, sky, noise = textures
    pal = metallic_palette(vrt, ids=L.NEIGHBOURS)
    svol = L.pair_source(pair)
    vol, dst = destination(vrt, engine, textures, dims, bricks, pal=pal)
    src = vrt.VoxelScene.from_dense(engine, svol, pal)
    try:
        size = L.SLAB_DIMS
        vol, res = stamp_checked(vrt, engine, dst, vol, pal, bricks, dims, src, svol, L.face_lo(dims, size), size, 0, True, f"{name} ids {pair}")
        exp = bc.assert_frame_equals_oracle(vrt, oracle, engine, dst, vol, pal, sky, noise, dims, f"{name} ids {pair}", METAL_PLANES)
        assert (exp["hit_id"] == pair[0]).any() and (exp["hit_id"] == pair[1]).any()
    finally:
        dst.destroy(); src.destroy()


# ---- group D ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bricks", [False, True], ids=["dense", "bricks"])
@pytest.mark.parametrize("s", [0, 1, 2], ids=["long-x", "long-y", "long-z"])
def test_stamps_with_a_side_of_512(vrt, engine, textures, s, bricks):
    pal = textures[0]
    svol, slo = L.long_source(s, bricks)
    size = L.long_size(s)
    src = bc.make_scene(vrt, engine, svol, pal, bricks, spare=None)
    try:
        for t in range(3):
            dims = L.long_dst_dims(t, bricks)
            rng = np.random.default_rng(7 + t)
            vol = ((rng.random(dims[::-1]) < 0.05) * rng.integers(1, 199, dims[::-1])).astype(np.uint8)
            dst = bc.make_scene(vrt, engine, vol, pal, bricks, spare=L.all_bricks_spare(vol) if bricks else None)
            try:
                for kind, dlo, orient, skip, noop in L.long_stamps(s, t, dims):
                    what = f"source long on {s} into {dims}: {kind} at {dlo} orient {orient}"
                    exp, res = R.stamp(vol, dlo, svol, slo, size, orient, skip)
                    assert (res[0] == 0) == noop, what
                    run(vrt, dst, bricks, {"stamp": (dlo, slo, size, orient, skip)}, res, exp, dims, what, src=src)
                    vol = exp
                bc.assert_state_equals_fresh(vrt, engine, dst, vol, pal, bricks, f"source long on {s} into {dims}")
            finally:
                dst.destroy()
        D, H, W = svol.shape
        assert (bc.whole(src, (W, H, D)) == svol).all()
    finally:
        src.destroy()


def test_stamp_of_512_by_512_onto_itself(vrt, engine, textures):
    pal = textures[0]
    vol = L.large_volume()
    sc = vrt.VoxelScene.from_dense(engine, vol, pal)
    try:
        exp, res = R.stamp(vol, *L.LARGE_STAMP[:1], vol, *L.LARGE_STAMP[1:])
        run(vrt, sc, False, {"stamp": L.LARGE_STAMP}, res, exp, L.LARGE_DIMS, "512 x 512 x 2 onto itself")
        bc.assert_state_equals_fresh(vrt, engine, sc, exp, pal, False, "512 x 512 x 2 onto itself")
    finally:
        sc.destroy()


# ---- group E ------------------------------------------------------------------------------------------------------------------------
def test_cpp_mirror_brush_and_stamp(vrt, tmp_path):
    """tests/native/brush_limits_main.cpp over host/voxels.hpp: VoxelScene::brush once, VoxelScene::stamp twice (one turned, with
    skipEmpty); the three results it prints and the scene it saves are the reference's"""
    src_cpp = os.path.join(ROOT, "tests", "native", "brush_limits_main.cpp")
    libdir = os.path.join(ROOT, "voxel-raytracing_amd", "csrc")
    exe = str(tmp_path / "brush_limits_main")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, src_cpp, "-L" + libdir, "-lvrt_hip", "-Wl,-rpath," + libdir], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    dims, sdims = (40, 24, 32), (17, 9, 11)
    rng = np.random.default_rng(5)
    vol = ((rng.random(dims[::-1]) < 0.2) * rng.integers(1, 199, dims[::-1])).astype(np.uint8)
    svol = ((rng.random(sdims[::-1]) < 0.5) * rng.integers(1, 256, sdims[::-1])).astype(np.uint8)
    a, b, out = tmp_path / "dst.u8", tmp_path / "src.u8", tmp_path / "out.vox"
    vol.tofile(a); svol.tofile(b)
    r = subprocess.run([exe, str(a), *map(str, dims), str(b), *map(str, sdims), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = [tuple(int(v) for v in line.split()[1:]) for line in r.stdout.splitlines() if line.startswith("result")]
    p = [41, 24, 33, 13, 9, 1024]                                                 # (what the program passes: see its source)
    v1, r1 = R.brush(vol, R.ELLIPSOID, R.ADD, p, 77)
    v2, r2 = R.stamp(v1, (-2, 3, 20), svol, (0, 0, 0), sdims, 0, False)
    v3, r3 = R.stamp(v2, (30, -4, 1), svol, (1, 2, 3), (15, 6, 7), 3 | 5 << 3, True)
    assert r1[0] > 0 and r2[0] > 0 and r3[0] > 0
    assert got == [(r[0], *r[1], *r[2]) for r in (r1, r2, r3)], (got, r1, r2, r3)
    loaded = vrt.vox_flatten_host(out.read_bytes())[0]
    assert loaded.shape == v3.shape and (loaded == v3).all()
