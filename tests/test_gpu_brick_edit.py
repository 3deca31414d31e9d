"""Edits of brick scenes on the GPU (vrt_scene_reserve_bricks, then vrt_scene_edit_box / vrt_scene_fill_box): after every edit
the scene's device structures equal those of vrt_scene_from_bricks of the numpy-edited volume -- canonically: which pool slot a
brick lies in is the one thing that may differ -- and what it renders equals the oracle's image of the edited volume and the
image of a dense scene edited by the same calls."""
import ctypes as C

import numpy as np
import pytest

from helpers import compare_planes, metallic_palette
from brick_edit_native import brick_edit_host, in_place
from test_gpu_scene_edit import apply_edit, edit_sequence, oracle_frame, reference_settings, smoke_like_scene

pytestmark = pytest.mark.gpu

GB = ["color8", "depth", "motion", "mask8", "position", "normal8"]
COUNTS = ["steps_primary", "steps_total", "rays_total"]
PTR = np.uint64(0xFFFFFF)


def brick_occupancy(vol):
    D, H, W = vol.shape
    return vol.reshape(D // 8, 8, H // 8, 8, W // 8, 8).any(axis=(1, 3, 5))


def brick_state(vrt, sc):
    K = vrt._capi
    return sc.debug_state(K.STATE_BENTRY), sc.debug_state(K.STATE_BPOOL), sc.debug_state(K.STATE_BFINE), np.sort(sc.debug_state(K.STATE_CELLS))


def assert_state_equals_fresh(vrt, engine, sc, vol, pal, what):
    grid, pool = vrt.synthetic.bricks_from_dense(vol)
    fresh = vrt.VoxelScene.from_bricks(engine, grid, pool, pal)
    try:
        (ea, pa, fa, ca), (eb, pb, fb, cb) = brick_state(vrt, sc), brick_state(vrt, fresh)
        assert ea.shape == eb.shape, (what, ea.shape, eb.shape)
        diff = np.flatnonzero((ea & ~PTR) != (eb & ~PTR))
        assert diff.size == 0, f"{what}: {diff.size} entries differ beside the pointer, first at padded index {int(diff[0])}: {int(ea[diff[0]]):#x} != {int(eb[diff[0]]):#x}"
        ptr_a, ptr_b = (ea & PTR).astype(np.int64), (eb & PTR).astype(np.int64)
        kind = lambda p: np.where(p == 0, 0, np.where(p == 0xFFFFFF, 2, 1))               # empty / occupied / border
        assert (kind(ptr_a) == kind(ptr_b)).all(), (what, "pointers")
        occ = kind(ptr_a) == 1
        assert int(occ.sum()) == pool.shape[0] and len(set(ptr_a[occ].tolist())) == int(occ.sum()), (what, "slots")
        assert int(ptr_a[occ].max(initial=0)) <= pa.shape[0], (what, "a pointer past the pool")
        assert (pa[ptr_a[occ] - 1] == pb[ptr_b[occ] - 1]).all(), (what, "ids")
        bad = np.flatnonzero((fa[ptr_a[occ] - 1] != fb[ptr_b[occ] - 1]).reshape(int(occ.sum()), 8 * 512).any(axis=1))
        assert bad.size == 0, f"{what}: the fine bytes of {bad.size} bricks differ, first at padded index {int(np.flatnonzero(occ)[bad[0]])}"
        assert ca.shape == cb.shape and (ca == cb).all(), (what, "cells")
    finally:
        fresh.destroy()


def brick_edit_sequence(rng, dims):
    """the kinds of tests/test_gpu_scene_edit.py and those only a brick scene knows"""
    W, H, D = dims
    seq = edit_sequence(rng, dims)
    extra = [("brick-aligned fill", [8, 16, 24], ([16, 8, 8], 21)),
             ("brick-aligned fill, two bricks deep", [W - 24, 0, D - 16], ([24, 16, 16], 22)),
             ("carve that empties whole bricks", [8, 16, 24], ([16, 8, 8], 0)),
             ("carve that empties bricks and cuts into others", [W - 28, 0, D - 20], ([28, 12, 20], 0)),
             ("a box straddling 8 bricks", [14, 22, 30], ([4, 4, 4], 23)),
             ("the same, other ids", [14, 22, 30], ([4, 4, 4], 24)),
             ("a box straddling 8 bricks, carved", [15, 23, 31], ([2, 2, 2], 0)),
             ("a box on a volume face", [0, 8, 8], ([3, 17, 9], 25)),
             ("a box on the opposite face", [W - 2, H - 9, 0], ([2, 9, 5], 26)),
             ("one voxel into an empty brick", [W // 2 + 1, H - 3, 2], ([1, 1, 1], 27)),
             ("and out again", [W // 2 + 1, H - 3, 2], ([1, 1, 1], 0))]
    # before the sequence's own "whole volume" edits, which end with an (almost) empty volume
    k = next(i for i, e in enumerate(seq) if e[0] == "whole volume, mixed")
    return seq[:k] + extra + seq[k:] + [("fill after the void", [W // 3, H // 3, D // 3], ([10, 9, 12], 31)),
                                       ("overwrite inside it", [W // 3 + 1, H // 3 + 1, D // 3 + 1], ([3, 3, 3], 32)),
                                       ("whole volume, mixed again", [0, 0, 0], ((rng.random((D, H, W)) < 0.002) * rng.integers(1, 200, (D, H, W))).astype(np.uint8))]


@pytest.mark.parametrize("dims", [(96, 64, 88), (160, 40, 48)])
def test_state_after_every_edit_equals_a_fresh_build(vrt, engine, dims):
    W, H, D = dims
    nb = (W // 8, H // 8, D // 8)
    rng = np.random.default_rng(W)
    vol = ((rng.random((D, H, W)) < 0.0015) * rng.integers(1, 200, (D, H, W))).astype(np.uint8)
    vol[D // 2:D // 2 + 10, H // 3:H // 3 + 8, W // 4:W // 4 + 30] = 40
    pal = metallic_palette(vrt)
    grid, pool = vrt.synthetic.bricks_from_dense(vol)
    sc = vrt.VoxelScene.from_bricks(engine, grid, pool, pal)
    sc.reserve_bricks(nb[0] * nb[1] * nb[2])
    assert_state_equals_fresh(vrt, engine, sc, vol, pal, "after the reservation")
    rule = brick_edit_host()
    seq = brick_edit_sequence(rng, dims)
    assert len(seq) >= 30
    paths = {"fine only": 0, "in place": 0, "full build": 0}
    for k, (kind, lo, what) in enumerate(seq):
        before = brick_occupancy(vol)
        n = apply_edit(sc, vol, lo, what)
        changed = bool((brick_occupancy(vol) != before).any())
        path = "fine only" if not changed else ("in place" if in_place(rule, nb, lo, n) else "full build")
        paths[path] += 1
        assert_state_equals_fresh(vrt, engine, sc, vol, pal, f"edit {k} ({kind}) lo {lo} size {n}: {path}")
    print(paths)
    assert min(paths.values()) >= 2, paths
    sc.destroy()


def test_render_after_edits_equals_the_oracle_and_the_dense_scene(vrt, oracle, engine):
    N, res = 96, (320, 192)
    vol, pal, sky, noise = smoke_like_scene(vrt, N)
    vol = vol.copy()
    grid, pool = vrt.synthetic.bricks_from_dense(vol)
    sc = vrt.VoxelScene.from_bricks(engine, grid, pool, pal, sky=sky, noise=noise)
    sd = vrt.VoxelScene.from_dense(engine, vol, pal, sky=sky, noise=noise)
    sc.reserve_bricks(pool.shape[0] + 400)
    st = reference_settings(vrt, res)
    cam = vrt.CameraController(position=(N / 2 + 0.3, N / 2 + 0.2, -0.83 * N))
    push = vrt.make_push(cam, (N, N, N), res, frame=3)
    names = GB + ["color_f", "hit_id"]
    stage, stage_d = vrt.GeometryStage(engine, st, sc, debug_planes=True), vrt.GeometryStage(engine, st, sd, debug_planes=True)
    g0 = stage.record(push); engine.synchronize()
    g0 = {k: v.copy() for k, v in g0.numpy().items()}
    hit = g0["hit_id"] != 0
    assert 0.1 < hit.mean() < 0.9 and (g0["rays_total"] > 6).any()
    ys, xs = np.nonzero(hit)
    k = np.argmin((ys - res[1] // 2) ** 2 + (xs - res[0] // 2) ** 2)
    hv = g0["hit_voxel"][ys[k], xs[k]].astype(int)
    lo = [max(0, int(hv[a]) - 3) for a in range(3)]
    edits = [("carve into an occluder", lo, ([min(7, N - lo[a]) for a in range(3)], 0))]
    edits.append(("slab in front of sky", [2, 2, 0], ([48, 38, 3], 210)))
    rng = np.random.default_rng(3)
    edits.append(("mixed", [40, 40, 30], ((rng.random((12, 14, 16)) < 0.4) * rng.integers(1, 256, (12, 14, 16))).astype(np.uint8)))
    for i, (kind, lo, what) in enumerate(edits):
        model = vol.copy()
        apply_edit(sc, vol, lo, what)
        apply_edit(sd, model, lo, what)
        assert (model == vol).all()
        gb = stage.record(push)
        den = vrt.DenoiserStage(engine, st).record(gb.color, gb.normal, gb.position).cpu().numpy()
        engine.synchronize()
        g = {k: v.copy() for k, v in gb.numpy().items()}
        gd = stage_d.record(push); engine.synchronize()
        nm = names + COUNTS
        exp = oracle_frame(oracle, vol, pal, sky, noise, push, st, nm)
        assert not compare_planes(g, exp, nm), (kind, "oracle")
        assert not compare_planes(g, gd.numpy(), nm), (kind, "dense scene")
        assert (g["color8"] != g0["color8"]).any(), kind
        assert (den == oracle.denoise(exp["color8"], exp["normal8"], exp["position"])).all(), kind
    assert ((g0["hit_id"] == 0) & (g["hit_id"] == 210)).any()
    sc.destroy(); sd.destroy()


def test_metal_appears(vrt, oracle, engine):
    """a brick scene without any metallic voxel renders through the kernel without the bounce loop; an edit that writes one must
    change that"""
    N, res = 64, (192, 128)
    vol = vrt.synthetic.floating_cubes(N, seed=2, count=60)
    vol[vol >= 200] = 7
    pal = vrt.synthetic.default_palette(metallic_ids=range(200, 256))
    sky, noise = vrt.synthetic.sky_gradient(64, 32), vrt.synthetic.blue_noise_standin(64)
    grid, pool = vrt.synthetic.bricks_from_dense(vol)
    sc = vrt.VoxelScene.from_bricks(engine, grid, pool, pal, sky=sky, noise=noise)
    sc.reserve_bricks(pool.shape[0] + 64)
    st = reference_settings(vrt, res)
    push = vrt.make_push(vrt.CameraController(position=(N / 2 + 0.3, N / 2 + 0.2, -0.8 * N)), (N, N, N), res, frame=1)
    wall = np.full((2, N // 2, N // 2), 230, np.uint8)
    apply_edit(sc, vol, [N // 4, N // 4, 0], wall)
    names = GB + ["color_f", "hit_id", "rays_total"]
    gb = vrt.GeometryStage(engine, st, sc, debug_planes=True).record(push); engine.synchronize()
    g = gb.numpy()
    exp = oracle_frame(oracle, vol, pal, sky, noise, push, st, names)
    assert (exp["hit_id"] == 230).any() and int(exp["rays_total"].max()) > 6
    assert not compare_planes(g, exp, names)
    sc.destroy()


def test_frame_loop_render_edit_render(vrt, oracle, engine):
    """render, edit, render on one context without a host synchronisation in between, then a batch of four; the sharded frame
    (8 simulated ranks) after the edit equals the unsharded one"""
    N, res = 64, (160, 192)
    vol, pal, sky, noise = smoke_like_scene(vrt, N)
    vol = vol.copy()
    old = vol.copy()
    grid, pool = vrt.synthetic.bricks_from_dense(vol)
    sc = vrt.VoxelScene.from_bricks(engine, grid, pool, pal, sky=sky, noise=noise)
    sc.reserve_bricks(pool.shape[0] + 100)
    st = reference_settings(vrt, res)
    cams = [vrt.CameraController(position=(N / 2 + 0.3 + 2 * i, N / 2 + 0.2, -0.83 * N)) for i in range(4)]
    pushes = [vrt.make_push(c, (N, N, N), res, frame=i) for i, c in enumerate(cams)]
    a, b = vrt.GeometryStage(engine, st, sc), vrt.GeometryStage(engine, st, sc)
    launch4 = vrt.GeometryStage(engine, st, sc).prepare_batch(4)
    ga = a.record(pushes[0])
    apply_edit(sc, vol, [20, 20, 8], ([24, 24, 10], 215))
    gb = b.record(pushes[0])
    gbs = launch4(pushes)
    engine.synchronize()
    assert not compare_planes(ga.numpy(), oracle_frame(oracle, old, pal, sky, noise, pushes[0], st, GB), GB)
    full = {n: v.copy() for n, v in gb.numpy().items()}
    assert not compare_planes(full, oracle_frame(oracle, vol, pal, sky, noise, pushes[0], st, GB), GB)
    assert (ga.numpy()["color8"] != full["color8"]).any()
    for i in range(4):
        assert not compare_planes(gbs[i].numpy(), oracle_frame(oracle, vol, pal, sky, noise, pushes[i], st, GB), GB), i
    stage = vrt.GeometryStage(engine, st, sc)
    merged = {n: np.zeros_like(full[n]) for n in GB}
    rows = np.arange(res[1])
    for rank in range(8):
        pn = stage.record(pushes[0], vrt.make_shard(rank, 8, 16)).numpy()
        engine.synchronize()
        own = ((rows // 16) % 8) == rank
        for n in GB:
            merged[n][own] = pn[n][own]
    assert not compare_planes(merged, full, GB)
    sc.destroy()


def test_edit_bricks_numpy_is_the_dense_edit(vrt):
    rng = np.random.default_rng(4)
    vol = ((rng.random((24, 32, 40)) < 0.004) * rng.integers(1, 200, (24, 32, 40))).astype(np.uint8)
    grid, pool = vrt.synthetic.bricks_from_dense(vol)
    for lo, shape, p in (([5, 6, 7], (9, 11, 13), 0.3), ([0, 0, 0], (24, 32, 40), 0.0), ([8, 8, 8], (8, 8, 8), 1.0), ([30, 20, 10], (3, 4, 5), 0.5)):
        ids = ((rng.random(shape) < p) * rng.integers(1, 200, shape)).astype(np.uint8)
        vol[lo[2]:lo[2] + shape[0], lo[1]:lo[1] + shape[1], lo[0]:lo[0] + shape[2]] = ids
        grid, pool = vrt.synthetic.edit_bricks(grid, pool, lo, ids)
        assert (vrt.synthetic.dense_from_bricks(grid, pool) == vol).all()
        assert pool.reshape(pool.shape[0], 512).any(axis=1).all() and int(grid.max(initial=0)) == pool.shape[0]


def test_config5_size_edit(vrt, oracle, engine):
    """BASELINE configs[4] (2048^3 in bricks, 3840x2160, the settings of tests/test_gpu_bricks.py::test_config5_sparse2048_4k): one
    40 x 48 x 56 mixed edit near the centre of the volume, three bands of rows against the oracle reading the edited bricks"""
    grid, pool = vrt.synthetic.sparse_brick_scene(2048, 0.015, seed=5)
    N = 2048
    pal = metallic_palette(vrt)
    sky, noise = vrt.synthetic.sky_gradient(256, 128), vrt.synthetic.blue_noise_standin(512)
    sc = vrt.VoxelScene.from_bricks(engine, grid, pool, pal, sky=sky, noise=noise)
    unreserved = sc.memory_bytes()
    sc.reserve_bricks(pool.shape[0] + 4096)
    reservation = sc.memory_bytes() - unreserved
    assert reservation >= 4096 * 4608 + 5 * 258 ** 3
    res = (3840, 2160)
    st = vrt.VoxelRenderSettings(targetResolution=res)
    st.fsrSetttings.enable = False
    st.traceSettings.maxRaySteps = 6144
    st.traceSettings.maxReflections = 4
    st.occlusionSettings.numSamples = 4
    pos, yaw, pitch = vrt.synthetic.default_camera_for(N, N, N)
    cam = vrt.CameraController(position=(pos[0] + 0.3, pos[1] + 0.2, pos[2]), yaw=yaw, pitch=pitch)
    push = vrt.make_push(cam, (N, N, N), res, frame=17)
    names = GB + ["hit_id", "hit_voxel", "rays_total", "steps_total"]
    stage = vrt.GeometryStage(engine, st, sc, debug_planes=True)
    g0 = stage.record(push); engine.synchronize()
    g0 = g0.numpy()
    before = g0["color8"].copy()
    rng = np.random.default_rng(8)
    ids = ((rng.random((40, 48, 56)) < 0.5) * rng.integers(1, 256, (40, 48, 56))).astype(np.uint8)      # [z, y, x]: 56 x 48 x 40 voxels
    # on the camera's axis, which runs through the centre of the volume, around the voxel the centre-most hit pixel sees: as far
    # into the volume as an edit can lie and still be seen
    ys, xs = np.nonzero(g0["hit_id"] != 0)
    k = np.argmin((ys - res[1] // 2) ** 2 + (xs - res[0] // 2) ** 2)
    hv = g0["hit_voxel"][ys[k], xs[k]].astype(int)
    lo = [min(max(0, int(hv[0]) - 28), N - 56), min(max(0, int(hv[1]) - 24), N - 48), min(max(0, int(hv[2]) - 20), N - 40)]
    assert abs(lo[0] + 28 - N // 2) < N // 8 and abs(lo[1] + 24 - N // 2) < N // 8, lo
    print("edit at", lo)
    sc.edit(lo, ids)
    grid, pool = vrt.synthetic.edit_bricks(grid, pool, lo, ids)
    g = stage.record(push); engine.synchronize()
    g = g.numpy()
    assert (g["color8"] != before).any()
    osn = oracle.OracleScene(None, pal, sky=sky, noise=noise, bricks=(grid, pool))
    for r0 in (4, 1078, 2150):
        exp = oracle.render_band(osn, push, oracle.params_from(st.to_c()), r0, r0 + 4, planes=names, nthreads=16)
        assert not compare_planes({n: g[n][r0:r0 + 4] for n in names}, exp, names), r0
    assert sc.memory_bytes() < 2 * (1 << 30) + reservation, (sc.memory_bytes(), reservation)
    sc.destroy()


def test_reservation_and_errors(vrt, engine):
    pal = metallic_palette(vrt)
    K, VrtError = vrt._capi, vrt._capi.VrtError
    l = vrt.lib()
    i3, u3 = C.c_int32 * 3, C.c_uint32 * 3

    def rc_and_message(fn, *args):
        rc = fn(*args)
        return rc, l.vrt_last_error().decode()
    vol = np.zeros((32, 40, 48), np.uint8)                        # 6 x 5 x 4 bricks
    vol[8:16, 8:16, 8:16] = 5; vol[9, 30, 40] = 201; vol[25:27, 3:5, 20:28] = 9
    grid, pool = vrt.synthetic.bricks_from_dense(vol)
    n0 = pool.shape[0]
    assert n0 == 4
    sky, noise = vrt.synthetic.sky_gradient(64, 32), vrt.synthetic.blue_noise_standin(64)
    sc = vrt.VoxelScene.from_bricks(engine, grid, pool, pal, sky=sky, noise=noise)
    st = vrt.VoxelRenderSettings(targetResolution=(128, 96))
    st.fsrSetttings.enable = False
    push = vrt.make_push(vrt.CameraController(position=(24.3, 20.2, -30.0)), (48, 40, 32), (128, 96), frame=2)
    names = GB + COUNTS
    stage = vrt.GeometryStage(engine, st, sc, debug_planes=True)
    g0 = stage.record(push); engine.synchronize()
    g0 = {k: v.copy() for k, v in g0.numpy().items()}
    assert (g0["hit_id"] != 0).any()
    # an unreserved scene refuses edits; a capacity below the occupied bricks is invalid; a dense scene has nothing to reserve
    rc, msg = rc_and_message(l.vrt_scene_fill_box, engine.ctx, sc.handle, i3(0, 0, 0), u3(2, 2, 2), 1)
    assert rc == 7 and "vrt_scene_fill_box" in msg
    rc, msg = rc_and_message(l.vrt_scene_reserve_bricks, engine.ctx, sc.handle, n0 - 1)
    assert rc == 1 and "vrt_scene_reserve_bricks" in msg
    rc, msg = rc_and_message(l.vrt_scene_reserve_bricks, engine.ctx, sc.handle, 0xFFFFFE)
    assert rc == 1 and "vrt_scene_reserve_bricks" in msg
    rc, msg = rc_and_message(l.vrt_scene_fill_box, engine.ctx, sc.handle, i3(0, 0, 0), u3(2, 2, 2), 1)
    assert rc == 7                                                # the refused reservations reserved nothing
    sd = vrt.VoxelScene.from_dense(engine, vol, pal)
    rc, msg = rc_and_message(l.vrt_scene_reserve_bricks, engine.ctx, sd.handle, 100)
    assert rc == 7 and "vrt_scene_reserve_bricks" in msg
    rc, msg = rc_and_message(l.vrt_scene_reserve_bricks, engine.ctx, None, 100)
    assert rc == 1
    for what in (K.STATE_BENTRY, K.STATE_BPOOL, K.STATE_BFINE):   # the brick selectors are a brick scene's, the dense ones a dense scene's
        with pytest.raises(VrtError):
            sd.debug_state(what)
    with pytest.raises(VrtError):
        sc.debug_state(K.STATE_DF)
    sd.destroy()
    base = sc.memory_bytes()
    assert sc.debug_state(K.STATE_BPOOL).shape == (n0, 512) and sc.debug_state(K.STATE_BFINE).shape == (n0, 8, 512)
    sc.reserve_bricks(n0 + 2)
    assert sc.debug_state(K.STATE_BPOOL).shape == (n0 + 2, 512) and sc.debug_state(K.STATE_BENTRY).shape == (8 * 7 * 6,)
    reserved = sc.memory_bytes()
    assert reserved >= base + 2 * 4608 + 5 * 8 * 7 * 6           # the reservation is counted
    g1 = stage.record(push); engine.synchronize()
    assert not compare_planes(g1.numpy(), g0, names)              # and renders as before
    assert_state_equals_fresh(vrt, engine, sc, vol, pal, "reserved")
    sc.reserve_bricks(n0)                                         # a smaller capacity that holds the bricks: allowed, nothing changes
    assert sc.memory_bytes() == reserved
    # box and NULL errors, as on a dense scene
    ids = np.zeros(8, np.uint8)
    for lo, size in (((47, 0, 0), (2, 1, 1)), ((0, -1, 0), (1, 1, 1)), ((0, 0, 32), (1, 1, 1)), ((0, 0, 0), (49, 1, 1)), ((4, 4, 4), (2, 0, 2))):
        rc, msg = rc_and_message(l.vrt_scene_edit_box, engine.ctx, sc.handle, i3(*lo), u3(*size), ids.ctypes.data_as(C.c_void_p))
        assert rc == 1 and "vrt_scene_edit_box" in msg, (lo, size, rc, msg)
        rc, msg = rc_and_message(l.vrt_scene_fill_box, engine.ctx, sc.handle, i3(*lo), u3(*size), 3)
        assert rc == 1 and "vrt_scene_fill_box" in msg, (lo, size, rc, msg)
    rc, msg = rc_and_message(l.vrt_scene_edit_box, engine.ctx, sc.handle, i3(0, 0, 0), u3(2, 2, 2), None)
    assert rc == 1 and "vrt_scene_edit_box" in msg
    rc, msg = rc_and_message(l.vrt_scene_fill_box, engine.ctx, sc.handle, None, u3(2, 2, 2), 1)
    assert rc == 1 and "vrt_scene_fill_box" in msg
    # an edit that needs three slots where two are free: refused, and nothing changed
    states = (K.STATE_BENTRY, K.STATE_BPOOL, K.STATE_BFINE, K.STATE_CELLS)
    snap = [sc.debug_state(w).copy() for w in states]
    rc, msg = rc_and_message(l.vrt_scene_fill_box, engine.ctx, sc.handle, i3(24, 16, 16), u3(24, 8, 8), 7)
    assert rc == 7 and "vrt_scene_fill_box" in msg and "vrt_scene_reserve_bricks" in msg, (rc, msg)
    for w, before in zip(states, snap):
        after = sc.debug_state(w)
        assert after.shape == before.shape and (after == before).all(), w
    g1 = stage.record(push); engine.synchronize()
    assert not compare_planes(g1.numpy(), g0, names)
    sc.reserve_bricks(n0 + 3)                                     # grow, and the same edit goes through
    sc.fill((24, 16, 16), (24, 8, 8), 7)
    vol[16:24, 16:24, 24:48] = 7
    assert_state_equals_fresh(vrt, engine, sc, vol, pal, "after growing")
    # slots are used again: 7 slots, bricks filled and emptied 40 times over, never more than 7 at once
    assert n0 + 3 == 7
    rng = np.random.default_rng(11)
    filled = 0
    for k in range(40):
        bx, by, bz = (int(rng.integers(0, 6)), int(rng.integers(0, 5)), int(rng.integers(0, 4)))
        if brick_occupancy(vol).sum() == 7 or (k % 3 == 2 and brick_occupancy(vol).any()):
            oz, oy, ox = (int(v[0]) for v in np.nonzero(brick_occupancy(vol)))          # empty the first occupied brick
            sc.fill((ox * 8, oy * 8, oz * 8), (8, 8, 8), 0)
            vol[oz * 8:oz * 8 + 8, oy * 8:oy * 8 + 8, ox * 8:ox * 8 + 8] = 0
        if not brick_occupancy(vol)[bz, by, bx]:
            filled += 1
        sc.fill((bx * 8 + 2, by * 8 + 1, bz * 8 + 3), (3, 4, 2), 30 + k)
        vol[bz * 8 + 3:bz * 8 + 5, by * 8 + 1:by * 8 + 5, bx * 8 + 2:bx * 8 + 5] = 30 + k
        assert brick_occupancy(vol).sum() <= 7
    assert filled > 7, filled
    assert_state_equals_fresh(vrt, engine, sc, vol, pal, "after reusing slots")
    assert sc.debug_state(K.STATE_BPOOL).shape == (7, 512)
    # one edit that empties bricks and fills as many others with no slot to spare takes the slots it frees
    while brick_occupancy(vol).sum() < 7:
        oz, oy, ox = (int(v[0]) for v in np.nonzero(~brick_occupancy(vol)))
        sc.fill((ox * 8, oy * 8, oz * 8), (1, 1, 1), 3)
        vol[oz * 8, oy * 8, ox * 8] = 3
    whole = np.zeros_like(vol)
    for oz, oy, ox in zip(*np.nonzero(~brick_occupancy(vol))):
        if np.count_nonzero(whole) < 7:
            whole[oz * 8 + 1, oy * 8 + 1, ox * 8 + 1] = 77
    sc.edit((0, 0, 0), whole)
    vol[:] = whole
    assert brick_occupancy(vol).sum() == 7
    assert_state_equals_fresh(vrt, engine, sc, vol, pal, "seven bricks moved by one edit")
    # trim drops the passes' scratch memory, never the reservation
    with_scratch = sc.memory_bytes()
    sc.trim()
    assert reserved < sc.memory_bytes() <= with_scratch
    sc.fill((0, 0, 0), (2, 2, 2), 9)
    vol[0:2, 0:2, 0:2] = 9
    assert_state_equals_fresh(vrt, engine, sc, vol, pal, "an edit after trim")
    g2 = stage.record(push); engine.synchronize()
    osn_vol = vol.copy()
    sd = vrt.VoxelScene.from_dense(engine, osn_vol, pal, sky=sky, noise=noise)
    gd = vrt.GeometryStage(engine, st, sd, debug_planes=True).record(push); engine.synchronize()
    assert not compare_planes(g2.numpy(), gd.numpy(), names)
    sd.destroy()
    sc.destroy()
