"""Every stage at the documented size limits (include/vrt.h) on the GPU, bit for bit against the oracle: the volumes, ray batches and
cameras of tests/extents_common.py, whose composition tests/test_extents_cpu.py has decided on the oracle alone (the same
conditions are asserted again here, on the records the comparison uses).
  needles        4096 (ragged: 4093) voxels along x, y or z: cells 0 .. 1023 of the occupied-cell list (x | y << 10 | z << 20: 1023
                 is the last value that fits), rows and columns as long as an axis may be;
  brick needles  512 bricks along an axis, as a dense scene and through vrt_scene_from_bricks: brick coordinates 0 .. 511, the same
                 packing, and mul24(bz, pbx * pby) over the padded grid;
  slabs          (W + 2)(H + 2) = 2^23 - 4096 and 2^23: the first carries nine fields and the 0xFF byte -- the look-up loops
                 (v_mad_i32_i24 with pw and pwh) and the 32-bit form of VRT_TRAVERSAL_DF (mul24) run at the largest slice they may
                 take; the second carries eight fields -- both are refused and the 64-bit march runs.  VoxelScene.memory_bytes says
                 which side a scene is on (fields_of below).
Budgets 1024 / 1025 are VRT_TRAVERSAL_AUTO's switch: up to 1024 the hand-written look-up loop, from 1025 on the general march."""
import ctypes as C

import numpy as np
import pytest

import extents_common as X
import scene_reference as R
from helpers import compare_planes, metallic_palette
from ray_query_common import oracle_records, planes_differ
from test_extents_cpu import frame_condition, needle_conditions, no_open_rays, slab_conditions
from test_gpu_brick_edit import assert_state_equals_fresh as brick_state_equals_fresh
from test_gpu_scene_edit import apply_edit, assert_state_equals_fresh

pytestmark = pytest.mark.gpu

GB = ["color8", "depth", "motion", "mask8", "position", "normal8"]
DBG = ["color_f", "hit_id", "hit_voxel", "hit_mask", "steps_primary", "steps_total", "rays_total"]
DBG_JUMP = ["color_f", "hit_id", "hit_voxel", "hit_mask", "rays_total"]            # JUMP / DFJ fetch counts are upper bounds
# what has been compared so far, printed once per test (as test_gpu_scene_build.py does); counted after the assertion it counts
TOTAL = {"rays": 0, "hits": 0, "frames": 0, "pixels": 0, "states": 0}
ids = lambda d: "x".join(str(v) for v in d) if isinstance(d, tuple) else str(d)


@pytest.fixture(scope="module")
def textures(vrt):
    return metallic_palette(vrt), vrt.synthetic.sky_gradient(64, 32), vrt.synthetic.blue_noise_standin(64)


@pytest.fixture(scope="module")
def expected(vrt, oracle, textures):
    """the oracle's records per (volume, direction, budget) and frames per (volume, camera, frame size, setting), computed once"""
    pal, sky, noise = textures
    vols, scenes, cache = {}, {}, {}

    def volume(dims):
        if dims not in vols:
            vols[dims] = X.slab_volume(dims) if dims[2] == 3 else X.needle_volume(dims)
            scenes[dims] = oracle.OracleScene(vols[dims], pal, sky=sky, noise=noise)
        return vols[dims]

    def records(dims, sign, ms):
        key = ("rays", dims, sign, ms)
        if key not in cache:
            volume(dims)
            s, d = X.slab_rays(dims) if sign == 0 else X.needle_rays(dims, sign)
            cache[key] = (s, d) + oracle_records(oracle, scenes[dims], s, d, ms)
        return cache[key]

    def frame(dims, cam, res, name, st):
        key = ("frame", dims, cam[0], res, name)
        if key not in cache:
            volume(dims)
            cache[key] = oracle.render(scenes[dims], X.push_of(vrt, dims, res, cam), oracle.params_from(st.to_c()), nthreads=8)
        return cache[key]

    def forget(dims):
        vols.pop(dims, None); scenes.pop(dims, None)
        for key in [k for k in cache if k[1] == dims]:
            del cache[key]
    return {"volume": volume, "records": records, "frame": frame, "forget": forget}


def fields_of(vrt, sc, dims, textures):
    """The clearance-field bytes of a dense scene out of VoxelScene.memory_bytes (vrt_scene_from_dense: voxels + fields + pyramid +
    palette, + 4 bytes per occupied cell; vrt_scene_memory: + 20 bytes per sky texel, 4 per noise texel, 1024), as (number of
    fields, bytes behind them)."""
    _, sky, noise = textures
    W, H, D = dims
    n = [-(-v // 4) for v in dims]; n1 = n[0] * n[1] * n[2]
    n = [-(-v // 4) for v in n]; n2 = n[0] * n[1] * n[2]
    n = [-(-v // 4) for v in n]; n3 = n[0] * n[1] * n[2]
    rest = W * H * D + (n1 + (n2 + 1) // 2 * 2 + (n3 + 1) // 2 * 2) * 8 + 256 * C.sizeof(vrt._capi.Material) + 4 * sc.debug_state(vrt._capi.STATE_CELLS).size
    rest += sky.shape[0] * sky.shape[1] * 20 + noise.shape[0] * noise.shape[1] * 4 + 1024
    return divmod(sc.memory_bytes() - rest, R.df_field_bytes(W, H, D))


def check_queries(scenes, s, d, ms, exp, what):
    got = {}
    for kind, sc in scenes.items():
        got[kind] = sc.trace_rays(s, d, ms)
        bad = planes_differ(got[kind], exp)
        assert bad.size == 0, (what, kind, ms, bad[:5], {k: a[bad[:3]] for k, a in got[kind].items()}, {k: a[bad[:3]] for k, a in exp.items()},
                               s[bad[:3]], d[bad[:3]])
        TOTAL["rays"] += len(s); TOTAL["hits"] += int((got[kind]["material"] != 0).sum())
        occ = sc.occluded(s, d, ms)
        assert (occ == (exp["material"] != 0)).all(), (what, kind, ms, np.flatnonzero(occ != (exp["material"] != 0))[:5])
    if "brick" in got:
        assert planes_differ(got["dense"], got["brick"]).size == 0, (what, ms)


def needle_queries(expected, scenes, dims):
    for sign in (1, -1):
        records = {}
        for ms in X.BUDGETS:                                      # 1024: the look-up loop; 1025, 5000: the general march
            s, d, exp, cls = expected["records"](dims, sign, ms)
            no_open_rays(s, d, dims)
            records[ms] = (exp, cls)
            check_queries(scenes, s, d, ms, exp, (dims, sign))
        needle_conditions(dims, sign, s, records)


def check_frames(vrt, engine, expected, scenes, dims, cams, traversals=("AUTO",), frames=X.FRAMES, only=None):
    """every camera x frame size x setting: the launch with debug planes and the plain six-target launch (tile tags, sky paths)
    equal the oracle's frame; a brick scene renders the plain launch and equals the oracle, hence the dense scene"""
    for cam in cams:
        for res in frames:
            push = X.push_of(vrt, dims, res, cam)
            for name, st in X.render_settings(vrt, res):
                if only is not None and name not in only:
                    continue
                exp = expected["frame"](dims, cam, res, name, st)
                frame_condition(exp["hit_id"], (dims, cam[0], res, name))
                for trav in traversals:
                    st.traceSettings.traversal = getattr(vrt, "TRAVERSAL_" + trav)
                    what = (dims, cam[0], res, name, trav)
                    g = vrt.GeometryStage(engine, st, scenes["dense"], debug_planes=True).record(push)
                    engine.synchronize()
                    bad = compare_planes(g.numpy(), exp, GB + (DBG_JUMP if trav in ("JUMP", "DFJ") else DBG))
                    assert not bad, (what, "debug planes", bad[:2])
                    plain = vrt.GeometryStage(engine, st, scenes["dense"]).record(push)
                    engine.synchronize()
                    plain = plain.numpy()
                    bad = compare_planes(plain, exp, GB)
                    assert not bad, (what, "six targets", bad[:2])
                    TOTAL["frames"] += 2; TOTAL["pixels"] += 2 * res[0] * res[1]
                st.traceSettings.traversal = vrt.TRAVERSAL_AUTO
                if "brick" in scenes:
                    pb = vrt.GeometryStage(engine, st, scenes["brick"]).record(push)
                    engine.synchronize()
                    pb = pb.numpy()
                    bad = compare_planes(pb, exp, GB)
                    assert not bad, (dims, cam[0], res, name, "brick scene", bad[:2])
                    assert not compare_planes(pb, plain, GB)
                    TOTAL["frames"] += 1; TOTAL["pixels"] += res[0] * res[1]


@pytest.mark.parametrize("dims", X.NEEDLES + X.RAGGED, ids=ids)
def test_needle_queries_and_frames(vrt, engine, expected, textures, dims):
    """a needle as a dense scene: cells 0 and 1023 are in its cell list; vrt_trace_rays / vrt_occluded_rays along the axis in both
    directions at 1024 (look-up loop), 1025 and 5000 (general march); four cameras x two frame sizes x three settings with
    VRT_TRAVERSAL_AUTO; on the 4096 needles DENSE, BITMASK, JUMP, DF and DFJ too (the small frame, the defaults at 1024 and at 5000)"""
    pal, sky, noise = textures
    vol = expected["volume"](dims)
    sc = vrt.VoxelScene.from_dense(engine, vol, pal, sky=sky, noise=noise)
    try:
        a = X.long_axis(dims)
        cells = sc.debug_state(vrt._capi.STATE_CELLS) >> np.uint32(10 * a) & np.uint32(1023)
        assert cells.min() == 0 and cells.max() == 1023 and fields_of(vrt, sc, dims, textures) == (9, 256)
        needle_queries(expected, {"dense": sc}, dims)
        check_frames(vrt, engine, expected, {"dense": sc}, dims, X.needle_cameras(dims))
        if dims in X.NEEDLES:
            check_frames(vrt, engine, expected, {"dense": sc}, dims, X.needle_cameras(dims), ("DENSE", "BITMASK", "JUMP", "DF", "DFJ"),
                         X.FRAMES[1:], ("defaults, 1024", "defaults, 5000"))
        print(f"{dims}: so far {TOTAL}")
    finally:
        sc.destroy()
        expected["forget"](dims)


@pytest.mark.parametrize("nb", X.BRICK_NEEDLES, ids=ids)
def test_brick_needle_queries_and_frames(vrt, engine, expected, textures, nb):
    """512 bricks along an axis, as a dense scene and through vrt_scene_from_bricks (brick coordinate 511 is in the cell list): the
    queries and the frames of both equal the oracle, and each other"""
    pal, sky, noise = textures
    dims = tuple(8 * n for n in nb)
    vol = expected["volume"](dims)
    grid, pool = vrt.synthetic.bricks_from_dense(vol)
    scenes = {"dense": vrt.VoxelScene.from_dense(engine, vol, pal, sky=sky, noise=noise),
              "brick": vrt.VoxelScene.from_bricks(engine, grid, pool, pal, sky=sky, noise=noise)}
    try:
        a = X.long_axis(dims)
        cells = scenes["brick"].debug_state(vrt._capi.STATE_CELLS) >> np.uint32(10 * a) & np.uint32(1023)
        assert cells.min() == 0 and cells.max() == 511
        needle_queries(expected, scenes, dims)
        check_frames(vrt, engine, expected, scenes, dims, X.needle_cameras(dims))
        print(f"{dims}: so far {TOTAL}")
    finally:
        for sc in scenes.values():
            sc.destroy()
        expected["forget"](dims)


@pytest.mark.parametrize("dims,fast", X.SLABS, ids=ids)
def test_slab_on_either_side_of_the_24bit_slice(vrt, engine, expected, textures, dims, fast):
    """(W + 2)(H + 2) = 2^23 - 4096: nine fields and the 0xFF byte, the look-up loops at 1024 and the 32-bit march (mul24) at 1025, the
    first budget that must take it, and at 5000; = 2^23: eight fields, the 64-bit march at all three.  Rays from all four corners along x, y and the diagonal, crossing slices in
    both z directions; a camera above the far corner and one inside it."""
    pal, sky, noise = textures
    vol = expected["volume"](dims)
    sc = vrt.VoxelScene.from_dense(engine, vol, pal, sky=sky, noise=noise)
    try:
        assert fields_of(vrt, sc, dims, textures) == ((9, 256) if fast else (8, 0)), (dims, fields_of(vrt, sc, dims, textures))
        records = {}
        for ms in X.BUDGETS:                                      # nine fields: look-up loop, then the 32-bit march from 1025 on
            s, d, exp, cls = expected["records"](dims, 0, ms)
            no_open_rays(s, d, dims)
            records[ms] = (exp, cls)
            check_queries({"dense": sc}, s, d, ms, exp, dims)
        slab_conditions(dims, records)
        check_frames(vrt, engine, expected, {"dense": sc}, dims, X.slab_cameras(dims))
        print(f"{dims}: so far {TOTAL}")
    finally:
        sc.destroy()
        expected["forget"](dims)


def far_end_edits(dims):
    """(kind, lo, (size, id)) at the far end of the long axis: a fill over its last six 4^3 cells, a carve at the same place, one
    voxel at the last coordinate, a box across the boundary of cells 1022 / 1023"""
    a = X.long_axis(dims)
    L = dims[a]

    def box(first, n, across):
        lo, size = [0, 0, 0], list(across)
        lo[a], size[a] = first, n
        return lo, size
    full = list(dims)
    lo1, n1 = box(L - 24, 24, full)
    lo3, n3 = box(L - 1, 1, [1, 1, 1]); lo3 = [lo3[b] if b == a else dims[b] // 2 for b in range(3)]
    lo4, n4 = box(4090, 4, [min(3, v) for v in dims])
    assert lo4[a] >> 2 == 1022 and (lo4[a] + 3) >> 2 == 1023
    return [("fill", lo1, (n1, 77)), ("carve", lo1, (n1, 0)), ("one voxel", lo3, (n3, X.METAL)), ("across cells 1022 / 1023", lo4, (n4, 33))]


@pytest.mark.parametrize("dims", X.NEEDLES + [tuple(8 * n for n in nb) for nb in X.BRICK_NEEDLES], ids=ids)
def test_edits_at_the_far_end(vrt, oracle, engine, textures, dims):
    """four edits at coordinate 4095 of a dense needle and of a brick needle (after reserve_bricks): after each the scene's state
    equals a fresh build of the numpy-edited volume, and the frame from beyond the far end then equals the oracle's"""
    pal, sky, noise = textures
    vol = X.needle_volume(dims).copy()
    bricks = all(v % 8 == 0 for v in dims)
    if bricks:
        grid, pool = vrt.synthetic.bricks_from_dense(vol)
        sc = vrt.VoxelScene.from_bricks(engine, grid, pool, pal, sky=sky, noise=noise)
        sc.reserve_bricks(pool.shape[0] + 8)
    else:
        sc = vrt.VoxelScene.from_dense(engine, vol, pal, sky=sky, noise=noise)
    try:
        for kind, lo, what in far_end_edits(dims):
            apply_edit(sc, vol, lo, what)
            (brick_state_equals_fresh if bricks else assert_state_equals_fresh)(vrt, engine, sc, vol, pal, f"{dims} {kind} lo {lo} size {what[0]}")
            TOTAL["states"] += 1
        cam = X.needle_cameras(dims)[0][:4] + (2.0,)                  # (the far cap is carved away: a closer look at what is left)
        res = X.FRAMES[0]
        name, st = X.render_settings(vrt, res)[0]
        push = X.push_of(vrt, dims, res, cam)
        exp = oracle.render(oracle.OracleScene(vol, pal, sky=sky, noise=noise), push, oracle.params_from(st.to_c()), nthreads=8)
        frame_condition(exp["hit_id"], (dims, "after the edits"))
        assert (exp["hit_id"] == 33).any()                            # the last edit is seen
        g = vrt.GeometryStage(engine, st, sc, debug_planes=not bricks).record(push)
        engine.synchronize()
        bad = compare_planes(g.numpy(), exp, GB + ([] if bricks else DBG))
        assert not bad, (dims, bad[:2])
        TOTAL["frames"] += 1; TOTAL["pixels"] += res[0] * res[1]
        print(f"{dims}: so far {TOTAL}")
    finally:
        sc.destroy()
