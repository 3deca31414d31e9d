"""Scene edits on the GPU (vrt_scene_edit_box / vrt_scene_fill_box): after every edit the scene's device structures equal, byte
for byte, those of a scene built by vrt_scene_from_dense from the numpy-edited volume (the cell list as a sorted array), and
what it renders equals the oracle's image of the edited volume."""
import ctypes as C

import numpy as np
import pytest

from helpers import compare_planes, metallic_palette
from edit_native import edit_host, in_place

pytestmark = pytest.mark.gpu

GB = ["color8", "depth", "motion", "mask8", "position", "normal8"]
COUNTS = ["steps_primary", "steps_total", "rays_total"]
STATES = ("VOX", "DF", "OCC1", "OCC2", "OCC3")


def assert_state_equals_fresh(vrt, engine, sc, vol, pal, what):
    fresh = vrt.VoxelScene.from_dense(engine, vol, pal)
    try:
        for n in STATES:
            a, b = sc.debug_state(getattr(vrt._capi, "STATE_" + n)), fresh.debug_state(getattr(vrt._capi, "STATE_" + n))
            assert a.shape == b.shape, (what, n, a.shape, b.shape)
            if not (a == b).all():
                i = np.flatnonzero(a != b)
                where = ""
                if n == "DF":
                    D, H, W = vol.shape
                    stride = ((W + 2) * (H + 2) * (D + 2) + 255) & ~255
                    o, r = divmod(int(i[0]), stride)
                    where = f" field {o} x {r % (W + 2) - 1} y {r // (W + 2) % (H + 2) - 1} z {r // ((W + 2) * (H + 2)) - 1}"
                raise AssertionError(f"{what}: {n} differs in {i.size} places, first at {int(i[0])}{where}: {int(a[i[0]])} != {int(b[i[0]])}")
        ca, cb = np.sort(sc.debug_state(vrt._capi.STATE_CELLS)), np.sort(fresh.debug_state(vrt._capi.STATE_CELLS))
        assert ca.shape == cb.shape and (ca == cb).all(), (what, "CELLS")
    finally:
        fresh.destroy()


def edit_sequence(rng, dims):
    """(kind, lo, ids[z, y, x] or (size, id)) -- at least 30 edits of every kind the feature knows"""
    W, H, D = dims
    seq = []

    def box(n, at=None):
        n = [min(n[a], dims[a]) for a in range(3)]
        lo = [int(rng.integers(0, dims[a] - n[a] + 1)) for a in range(3)] if at is None else [min(max(0, at[a]), dims[a] - n[a]) for a in range(3)]
        return lo, n
    for k in range(6):                                            # fills, carves, overwrites, mixtures somewhere inside
        lo, n = box([int(rng.integers(1, 24)) for _ in range(3)])
        seq.append(("fill", lo, (n, int(rng.integers(1, 200)))))
        lo2, n2 = box([int(rng.integers(1, 12)) for _ in range(3)], at=[lo[a] + int(rng.integers(-4, 8)) for a in range(3)])
        seq.append(("carve", lo2, (n2, 0)))
        seq.append(("overwrite", lo, (n, int(rng.integers(1, 200)))))          # (mostly) the same occupancy, other ids
        lo3, n3 = box([int(rng.integers(2, 20)) for _ in range(3)])
        seq.append(("mixed", lo3, ((rng.random((n3[2], n3[1], n3[0])) < 0.3) * rng.integers(1, 200, (n3[2], n3[1], n3[0]))).astype(np.uint8)))
    for k in range(4):                                            # single voxels
        lo, n = box([1, 1, 1])
        seq.append(("voxel", lo, (n, int(k % 2) * 7)))
    for corner in ((0, 0, 0), (W, H, D), (0, H, 0), (W, 0, D)):   # corners, then edges and faces
        lo, n = box([5, 4, 6], at=corner)
        seq.append(("corner", lo, (n, 9)))
    lo, n = box([3, 3, D], at=(0, H, 0)); seq.append(("edge", lo, (n, 11)))
    lo, n = box([W, 2, 2], at=(0, 0, D)); seq.append(("edge carve", lo, (n, 0)))
    lo, n = box([2, 7, 9], at=(W, H // 3, D // 3)); seq.append(("face", lo, (n, 12)))
    lo, n = box([6, 2, 5], at=(W // 2, 0, D // 2)); seq.append(("face", lo, (n, 13)))
    lo, n = box([140, 1, 1], at=(3, H // 2, 10)); seq.append(("wider than the cap", lo, (n, 14)))
    lo, n = box([140, 2, 3], at=(3, H // 2, 10)); seq.append(("wider than the cap, carve", lo, (n, 0)))
    seq.append(("whole volume, mixed", [0, 0, 0], ((rng.random((D, H, W)) < 0.01) * rng.integers(1, 200, (D, H, W))).astype(np.uint8)))
    seq.append(("whole volume, empty", [0, 0, 0], ([W, H, D], 0)))
    lo, n = box([1, 1, 1], at=(W // 2, H // 2, D // 3))
    seq.append(("empty -> one voxel", lo, (n, 5)))               # every open cell behind it closes ...
    seq.append(("one voxel -> empty", lo, (n, 0)))               # ... and opens again
    lo, n = box([1, 1, 1], at=(0, 0, 0))
    seq.append(("empty -> corner voxel", lo, (n, 6)))
    lo, n = box([9, 9, 9]); seq.append(("fill into the void", lo, (n, 3)))
    seq.append(("corner voxel -> empty", [0, 0, 0], ([1, 1, 1], 0)))
    return seq


def apply_edit(sc, vol, lo, what):
    if isinstance(what, tuple):
        n, vid = what
        vol[lo[2]:lo[2] + n[2], lo[1]:lo[1] + n[1], lo[0]:lo[0] + n[0]] = vid
        sc.fill(lo, n, vid)
        return n
    d, h, w = what.shape
    vol[lo[2]:lo[2] + d, lo[1]:lo[1] + h, lo[0]:lo[0] + w] = what
    sc.edit(lo, what)
    return [w, h, d]


@pytest.mark.parametrize("dims", [(100, 60, 90), (300, 40, 150), (4096, 9, 12), (9, 12, 4096)])
def test_state_after_every_edit_equals_a_fresh_build(vrt, engine, dims):
    W, H, D = dims
    rng = np.random.default_rng(W)
    vol = ((rng.random((D, H, W)) < 0.004) * rng.integers(1, 200, (D, H, W))).astype(np.uint8)
    vol[D // 2:D // 2 + 10, H // 3:H // 3 + 8, W // 4:W // 4 + 30] = 40
    pal = metallic_palette(vrt)
    sc = vrt.VoxelScene.from_dense(engine, vol, pal)
    rule = edit_host()
    seq = edit_sequence(rng, dims)
    assert len(seq) >= 30
    paths = {True: 0, False: 0}
    for k, (kind, lo, what) in enumerate(seq):
        n = apply_edit(sc, vol, lo, what)
        paths[in_place(rule, dims, lo, n)] += 1
        assert_state_equals_fresh(vrt, engine, sc, vol, pal, f"edit {k} ({kind}) lo {lo} size {n}")
    assert paths[True] >= 25 and paths[False] >= 2, paths         # both the in-place path and the full rebuild ran
    assert (sc.download()[0] == vol).all()
    sc.destroy()


def test_rebuild_rule_both_sides_give_the_fresh_state(vrt, engine):
    """one edit just on either side of the rule of csrc/vrt_edit.h (in place while the eight R_o hold fewer than 4 W H D cells)"""
    dims = (96, 80, 72)
    W, H, D = dims
    rng = np.random.default_rng(5)
    vol = ((rng.random((D, H, W)) < 0.01) * rng.integers(1, 200, (D, H, W))).astype(np.uint8)
    pal = metallic_palette(vrt)
    sc = vrt.VoxelScene.from_dense(engine, vol, pal)
    rule = edit_host()
    # a box of side n in the middle: the sum over the octants is the product over the axes of (dim + n); find the n where the rule turns
    n = next(n for n in range(1, 72) if not in_place(rule, dims, [(W - n) // 2, (H - n) // 2, (D - n) // 2], [n] * 3))
    assert 2 < n < 72
    for m, expect in ((n - 1, True), (n, False)):
        lo = [(W - m) // 2, (H - m) // 2, (D - m) // 2]
        assert in_place(rule, dims, lo, [m] * 3) == expect
        ids = ((rng.random((m, m, m)) < 0.2) * rng.integers(1, 200, (m, m, m))).astype(np.uint8)
        apply_edit(sc, vol, lo, ids)
        assert_state_equals_fresh(vrt, engine, sc, vol, pal, f"side {m}, in place {expect}")
    sc.destroy()


def smoke_like_scene(vrt, N=96, metallic=True):
    vol = vrt.synthetic.floating_cubes(N, seed=1, count=120)
    pal = vrt.synthetic.default_palette(metallic_ids=range(200, 256)) if metallic else vrt.synthetic.default_palette(metallic_ids=())
    return vol, pal, vrt.synthetic.sky_gradient(64, 32), vrt.synthetic.blue_noise_standin(64)


def reference_settings(vrt, res):
    st = vrt.VoxelRenderSettings(targetResolution=res)           # AO 4, shadows, 5 bounces: the reference's defaults
    st.fsrSetttings.enable = False
    return st


def oracle_frame(oracle, vol, pal, sky, noise, push, st, names):
    return oracle.render(oracle.OracleScene(vol, pal, sky=sky, noise=noise), push, oracle.params_from(st.to_c()), planes=names, nthreads=8)


def test_render_after_edits_equals_the_oracle(vrt, oracle, engine):
    N, res = 96, (320, 192)
    vol, pal, sky, noise = smoke_like_scene(vrt, N)
    sc = vrt.VoxelScene.from_dense(engine, vol, pal, sky=sky, noise=noise)
    st = reference_settings(vrt, res)
    cam = vrt.CameraController(position=(N / 2 + 0.3, N / 2 + 0.2, -0.83 * N))
    push = vrt.make_push(cam, (N, N, N), res, frame=3)
    names = GB + ["color_f", "hit_id"]
    stage = vrt.GeometryStage(engine, st, sc, debug_planes=True)
    g0 = stage.record(push); engine.synchronize()
    g0 = {k: v.copy() for k, v in g0.numpy().items()}
    hit = g0["hit_id"] != 0
    assert 0.1 < hit.mean() < 0.9 and (g0["rays_total"] > 6).any()                  # sky blocks, tagged blocks and bounces all occur
    # (1) carve into an occluder: the box around the voxel the centre-most hit pixel sees
    ys, xs = np.nonzero(hit)
    k = np.argmin((ys - res[1] // 2) ** 2 + (xs - res[0] // 2) ** 2)
    hv = g0["hit_voxel"][ys[k], xs[k]].astype(int)
    lo = [max(0, int(hv[a]) - 3) for a in range(3)]
    edits = [("carve into an occluder", lo, ([min(7, N - lo[a]) for a in range(3)], 0))]
    # (2) geometry in front of sky: a metallic slab near the camera-side wall, over a corner of the frame that saw only sky
    edits.append(("slab in front of sky", [2, 2, 0], ([48, 38, 3], 210)))
    # (3) a mixed box in the middle of the volume
    rng = np.random.default_rng(3)
    edits.append(("mixed", [40, 40, 30], ((rng.random((12, 14, 16)) < 0.4) * rng.integers(1, 256, (12, 14, 16))).astype(np.uint8)))
    for i, (kind, lo, what) in enumerate(edits):
        apply_edit(sc, vol, lo, what)
        last = i == len(edits) - 1
        gb = stage.record(push)
        den = vrt.DenoiserStage(engine, st).record(gb.color, gb.normal, gb.position).cpu().numpy()
        engine.synchronize()
        g = gb.numpy()
        nm = names + (COUNTS if last or i == 0 else [])               # the count planes march the rebuilt second set of fields
        exp = oracle_frame(oracle, vol, pal, sky, noise, push, st, nm)
        assert not compare_planes(g, exp, nm), kind
        assert (g["color8"] != g0["color8"]).any(), kind
        assert (den == oracle.denoise(exp["color8"], exp["normal8"], exp["position"])).all(), kind
    assert ((g0["hit_id"] == 0) & (g["hit_id"] == 210)).any()    # the slab covers what was sky
    sc.destroy()


def test_metal_appears(vrt, oracle, engine):
    """a scene without any metallic voxel renders through the kernel without the bounce loop; an edit that writes one must
    change that"""
    N, res = 64, (192, 128)
    vol = vrt.synthetic.floating_cubes(N, seed=2, count=60)
    vol[vol >= 200] = 7                                           # nothing metallic in it
    pal = vrt.synthetic.default_palette(metallic_ids=range(200, 256))
    sky, noise = vrt.synthetic.sky_gradient(64, 32), vrt.synthetic.blue_noise_standin(64)
    sc = vrt.VoxelScene.from_dense(engine, vol, pal, sky=sky, noise=noise)
    st = reference_settings(vrt, res)
    push = vrt.make_push(vrt.CameraController(position=(N / 2 + 0.3, N / 2 + 0.2, -0.8 * N)), (N, N, N), res, frame=1)
    wall = np.full((2, N // 2, N // 2), 230, np.uint8)            # [z, y, x]: a mirror facing the camera
    apply_edit(sc, vol, [N // 4, N // 4, 0], wall)
    names = GB + ["color_f", "hit_id", "rays_total"]
    gb = vrt.GeometryStage(engine, st, sc, debug_planes=True).record(push); engine.synchronize()
    g = gb.numpy()
    exp = oracle_frame(oracle, vol, pal, sky, noise, push, st, names)
    assert (exp["hit_id"] == 230).any() and int(exp["rays_total"].max()) > 6           # the mirror is seen and bounces
    assert not compare_planes(g, exp, names)
    sc.destroy()


def test_frame_loop_render_edit_render(vrt, oracle, engine):
    """render, edit, render on one context without a host synchronisation in between: the first image is the old volume's, the
    second the new one's; once more with a batch of four frames after the edit"""
    N, res = 64, (160, 96)
    vol, pal, sky, noise = smoke_like_scene(vrt, N)
    vol = vol.copy()
    old = vol.copy()
    sc = vrt.VoxelScene.from_dense(engine, vol, pal, sky=sky, noise=noise)
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
    assert not compare_planes(gb.numpy(), oracle_frame(oracle, vol, pal, sky, noise, pushes[0], st, GB), GB)
    assert (ga.numpy()["color8"] != gb.numpy()["color8"]).any()
    for i in range(4):
        assert not compare_planes(gbs[i].numpy(), oracle_frame(oracle, vol, pal, sky, noise, pushes[i], st, GB), GB), i
    sc.destroy()


def test_edit_of_a_volume_past_the_32bit_field_limit(vrt, oracle, engine):
    """the 832^3 scene of tests/test_gpu_configs.py: 64-bit field indices, no field 8.  One edit, checked by bands of rows"""
    N = 832
    vol = vrt.synthetic.sparse_bricks(N, 8, 0.004, seed=9)
    pal = metallic_palette(vrt)
    sc = vrt.VoxelScene.from_dense(engine, vol, pal)
    res = (640, 360)
    st = vrt.VoxelRenderSettings(targetResolution=res)
    st.fsrSetttings.enable = False
    st.traceSettings.maxRaySteps = 3000
    st.traceSettings.maxReflections = 1
    st.occlusionSettings.numSamples = 1
    pos, yaw, pitch = vrt.synthetic.default_camera_for(N, N, N)
    cam = vrt.CameraController(position=(pos[0] + 0.3, pos[1] + 0.2, pos[2]), yaw=yaw, pitch=pitch)
    push = vrt.make_push(cam, (N, N, N), res, frame=2)
    names = GB + ["hit_id", "hit_voxel", "steps_total", "rays_total"]
    stage = vrt.GeometryStage(engine, st, sc, debug_planes=True)
    before = stage.record(push); engine.synchronize()
    before = before.numpy()["color8"].copy()
    rng = np.random.default_rng(8)
    ids = ((rng.random((40, 48, 56)) < 0.5) * rng.integers(1, 256, (40, 48, 56))).astype(np.uint8)
    assert in_place(edit_host(), (N, N, N), [380, 390, 400], [56, 48, 40])
    apply_edit(sc, vol, [380, 390, 400], ids)
    gb = stage.record(push); engine.synchronize()
    g = gb.numpy()
    assert (g["color8"] != before).any()
    osn = oracle.OracleScene(vol, pal)
    for r0 in (40, 176, 300):
        exp = oracle.render_band(osn, push, oracle.params_from(st.to_c()), r0, r0 + 4, planes=names, nthreads=8)
        assert not compare_planes({n: g[n][r0:r0 + 4] for n in names}, exp, names), r0
    sc.destroy()


def test_errors(vrt, engine):
    pal = metallic_palette(vrt)
    vol = vrt.synthetic.floating_cubes(32, seed=1, count=10)
    sc = vrt.VoxelScene.from_dense(engine, vol, pal)
    l, VrtError = vrt.lib(), vrt._capi.VrtError
    i3, u3 = C.c_int32 * 3, C.c_uint32 * 3
    ids = np.zeros(8, np.uint8)

    def rc_and_message(fn, *args):
        rc = fn(*args)
        return rc, l.vrt_last_error().decode()
    for lo, size in (((31, 0, 0), (2, 1, 1)), ((0, -1, 0), (1, 1, 1)), ((0, 0, 32), (1, 1, 1)), ((0, 0, 0), (33, 1, 1)), ((4, 4, 4), (2, 0, 2))):
        rc, msg = rc_and_message(l.vrt_scene_edit_box, engine.ctx, sc.handle, i3(*lo), u3(*size), ids.ctypes.data_as(C.c_void_p))
        assert rc == 1 and "vrt_scene_edit_box" in msg, (lo, size, rc, msg)
        rc, msg = rc_and_message(l.vrt_scene_fill_box, engine.ctx, sc.handle, i3(*lo), u3(*size), 3)
        assert rc == 1 and "vrt_scene_fill_box" in msg, (lo, size, rc, msg)
    rc, msg = rc_and_message(l.vrt_scene_edit_box, engine.ctx, sc.handle, i3(0, 0, 0), u3(2, 2, 2), None)
    assert rc == 1 and "vrt_scene_edit_box" in msg
    rc, msg = rc_and_message(l.vrt_scene_fill_box, engine.ctx, sc.handle, None, u3(2, 2, 2), 1)
    assert rc == 1 and "vrt_scene_fill_box" in msg
    rc, msg = rc_and_message(l.vrt_scene_fill_box, engine.ctx, None, i3(0, 0, 0), u3(2, 2, 2), 1)
    assert rc == 1 and "vrt_scene_fill_box" in msg
    with pytest.raises(VrtError):
        sc.fill((0, 0, 0), (0, 1, 1), 1)
    assert (sc.download()[0] == vol).all()                        # a refused edit changes nothing
    base = sc.memory_bytes()
    sc.fill((3, 3, 3), (4, 4, 4), 9)
    assert sc.memory_bytes() >= base                              # the passes' scratch memory is counted ...
    sc.trim()
    vol[3:7, 3:7, 3:7] = 9
    fresh = vrt.VoxelScene.from_dense(engine, vol, pal)
    assert sc.memory_bytes() == fresh.memory_bytes()              # ... and given back; the cell list's bytes follow the edit
    fresh.destroy()
    sc.destroy()
    grid = np.zeros((4, 4, 4), np.uint32); grid[1, 1, 1] = 1
    bs = vrt.VoxelScene.from_bricks(engine, grid, np.full((1, 8, 8, 8), 5, np.uint8), pal)
    rc, msg = rc_and_message(l.vrt_scene_fill_box, engine.ctx, bs.handle, i3(0, 0, 0), u3(2, 2, 2), 1)
    assert rc == 7 and "vrt_scene_fill_box" in msg
    rc, msg = rc_and_message(l.vrt_scene_edit_box, engine.ctx, bs.handle, i3(0, 0, 0), u3(2, 2, 2), ids.ctypes.data_as(C.c_void_p))
    assert rc == 7 and "vrt_scene_edit_box" in msg
    bs.destroy()
