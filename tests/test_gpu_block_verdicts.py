"""The block verdicts of the primary-only kernels (csrc/vrt_span.h block_verdict_byte; k_block_verdicts behind k_tile_tags; the
waves of k_primary MODE 1 read their span's word) on the GPU, at the smallest shapes at which they can go wrong.  Every frame is
compared bit for bit, in the reference's six targets, with the oracle.

  widths 8, 24, 32, 40, 72, 100 (no span at all; cut spans; a width that is no multiple of 8) x heights 8 and 13
  cameras: every block sky, every block hit, and a sweep that puts one occupied block into each of the four roles of an
           otherwise all-sky span (asserted from the oracle's hit_id)
  launch shapes: one frame in the kernel arguments, three in the arguments, twelve in the slot table, 260 frames of 40x16 through
           vrt_render_geometry_slots (the second launch); two shards of a 40x32 frame with 16-row strips
  switches: sky_span = 0; tile_tags = 0 (a launch without tags: what a scene without a cell list gets); tags_async 1 and 2
  after box edits that add and remove the only occupied cell under a span
  six unsynchronised table launches with different poses behind a stalled stream (the fifth takes the ring slot of the first,
  every launch the verdict buffer of the launch before last)

Launches with their slots in the table take the verdict pass; launches with their slots in the kernel arguments (one frame, three
frames) keep the per-wave verdict and launch nothing more -- both forms have to give the oracle's frames.

The verdict buffer has no read-back: the images carry it (a wrong bit 0 traces a sky block -- same picture -- or skips an occupied
one -- a hole; a wrong bit 1 stores rows of the wrong pixels); the bytes themselves are pinned by tests/test_block_verdicts_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import launch_shapes_common as lsc
from helpers import camera_push, compare_planes, metallic_palette
from test_gpu_k1_diet import _stage_batch
from test_gpu_launch_shapes import Planes, _stall
from test_gpu_sky_span import ORACLE, SIX, _frames, _noise_sky, _same

pytestmark = pytest.mark.gpu

DIMS = (32, 32, 32)
SIX_ORACLE = [k for k in ORACLE if k in SIX]
WIDTHS, HEIGHTS = (8, 24, 32, 40, 72, 100), (8, 13)


def _volume():
    """one 4^3 cube in an empty 32^3 volume: from far away it covers a block or two"""
    vol = np.zeros((32, 32, 32), np.uint8)
    vol[14:18, 14:18, 14:18] = 7
    return vol


@pytest.fixture(scope="module")
def cube(vrt, oracle, engine):
    vol, pal = _volume(), metallic_palette(vrt)
    sky, noise = _noise_sky(256, 128, 5), vrt.synthetic.blue_noise_standin(32)
    sc = vrt.VoxelScene.from_dense(engine, vol, pal, sky=sky, noise=noise)
    yield sc, oracle.OracleScene(vol, pal, sky=sky, noise=noise)
    sc.destroy()


def _pose(vrt, res, kind, f, pitch=0.0):
    """kind "sky": the cube lies 70 degrees off the axis, in front of the camera plane and outside every frame; "hit": the camera
    stands in front of the cube and every ray hits it; "sweep": from 60 voxels away the cube is a few pixels wide, and the camera
    turns so that it stands in the f-th of twelve equal parts of the frame's width (of its first 96 columns)"""
    if kind == "sky":
        return camera_push(vrt, DIMS, res, (16.0, 16.0, -60.0), 160.0, 0.0, frame=f)
    if kind == "hit":
        return camera_push(vrt, DIMS, res, (16.0, 16.0, 13.0), 90.0, 0.0, frame=f)
    W = res[0]
    sx = 2.0 * ((f % 12 + 0.5) * min(W, 96) / 12.0) / W - 1.0
    return camera_push(vrt, DIMS, res, (16.0, 16.0, -44.0), 90.0 + float(np.degrees(np.arctan(sx))), pitch, frame=f)


def _expected(oracle, osn, st, pushes):
    return [oracle.render(osn, p, oracle.params_from(st.to_c()), planes=ORACLE, nthreads=8) for p in pushes]


def _single_roles(hit_id):
    """roles (0 .. 3) of the blocks that are the only block with a hit in a whole 32x8 span"""
    H, W = hit_id.shape[:2]
    hit = hit_id.reshape(H, W) != 0
    roles = set()
    for y in range(0, H, 8):
        for x in range(0, W - 31, 32):
            blocks = [bool(hit[y:y + 8, x + 8 * k:x + 8 * k + 8].any()) for k in range(4)]
            if sum(blocks) == 1:
                roles.add(blocks.index(True))
    return roles


def _six_planes(vrt, engine, n, res):
    """n poisoned frames that hold the reference's six targets only"""
    out = Planes(vrt, engine.torch_device, n, res)
    for f in range(n):
        out.c[f].hit_id = None
    return out


def _same_typed(got, f, exp, what):
    bad = compare_planes(Planes.typed(got, f), exp, SIX_ORACLE)
    assert not bad, (what, bad)


def _check(got, exp, what):
    for f in range(len(got)):
        _same(got[f], exp[f], SIX_ORACLE, what + (f,))
        assert not got[f]["motion"].any(), what + (f,)


@pytest.mark.parametrize("kind", ["sky", "hit", "sweep"])
@pytest.mark.parametrize("H", HEIGHTS)
@pytest.mark.parametrize("W", WIDTHS)
def test_widths_cameras_and_launch_shapes(vrt, oracle, engine, cube, W, H, kind):
    sc, osn = cube
    res = (W, H)
    st = vrt.VoxelRenderSettings.primary_only(res)
    pushes = [_pose(vrt, res, kind, f) for f in range(12)]
    exp = _expected(oracle, osn, st, pushes)
    hit = np.stack([e["hit_id"].reshape(H, W) != 0 for e in exp])
    if kind == "sky":
        assert not hit.any()
    if kind == "hit":
        assert hit.all()
    if kind == "sweep" and W >= 72:
        roles = set().union(*[_single_roles(e["hit_id"]) for e in exp])
        assert roles == {0, 1, 2, 3}, roles
    _check(_frames(vrt, engine, sc, st, pushes[:1], 1, SIX), exp[:1], (res, kind, "one frame"))
    _check(_stage_batch(vrt, engine, sc, st, pushes[:3], 1), exp[:3], (res, kind, "3 in the arguments"))
    _check(_stage_batch(vrt, engine, sc, st, pushes, 1), exp, (res, kind, "12 in the table"))


@pytest.mark.parametrize("switch", ["sky_span0", "no_tags", "tags_async1", "tags_async2"])
def test_switches(vrt, oracle, engine, cube, switch):
    """table launches with sky_span = 0 and without tags still read verdict bytes (bit 1 clear; bit 0 from the box alone), and with
    tags_async their verdicts are made behind the tags on the second stream; the launches with their slots in the kernel arguments
    work their verdicts out per wave under the same switches"""
    sc, osn = cube
    for res in ((100, 13), (40, 8)):
        st = vrt.VoxelRenderSettings.primary_only(res)
        pushes = [_pose(vrt, res, "sweep", f) for f in range(12)]
        exp = _expected(oracle, osn, st, pushes)
        span, tags = (0, 1) if switch == "sky_span0" else ((1, 0) if switch == "no_tags" else (1, 1))
        old = engine.option("tags_async")
        if switch.startswith("tags_async"):
            engine.set_option("tags_async", int(switch[-1]))
        try:
            for rounds in range(2):                                # (twice: both tag buffers, both verdict buffers)
                _check(_frames(vrt, engine, sc, st, pushes[:1], span, SIX, tile_tags=tags), exp[:1], (res, switch, "one frame", rounds))
                _check(_stage_batch(vrt, engine, sc, st, pushes[:3], span, tags), exp[:3], (res, switch, "3 in the arguments", rounds))
                _check(_stage_batch(vrt, engine, sc, st, pushes, span, tags), exp, (res, switch, "12 in the table", rounds))
        finally:
            engine.set_option("tags_async", old)


def test_two_shards_of_a_40x32_frame(vrt, oracle, engine, cube):
    """ranks 0 and 1 of a 2-rank split with 16-row strips: each rank's rows equal the oracle's, in the kernel arguments and in the table"""
    sc, osn = cube
    res = (40, 32)
    st = vrt.VoxelRenderSettings.primary_only(res)
    pushes = [_pose(vrt, res, "sweep", f, pitch=10.0 * (f % 3 - 1)) for f in range(12)]        # (the cube in either half and between)
    exp = _expected(oracle, osn, st, pushes)
    assert any((e["hit_id"][:16] != 0).any() for e in exp) and any((e["hit_id"][16:] != 0).any() for e in exp)
    for rank in (0, 1):
        rows = slice(16 * rank, 16 * rank + 16)
        for n in (1, 3, 12):
            got = _frames(vrt, engine, sc, st, pushes[:n], 1, SIX, shard=vrt._capi.Shard(rank, 2, 16))
            for f in range(n):
                _same(got[f], exp[f], SIX_ORACLE, ("shard", rank, n, f), rows=rows)


def test_260_frames_through_slots(vrt, oracle, engine, cube):
    """vrt_render_geometry_slots, 260 frames of 40x16 (a launch of 256 and one of 4: the second reads the other verdict buffer, laid
    out for another n_frames), frame f as rank f % 2 of a 2-rank split with 16-row strips: rank 0 owns the frame's one strip, rank
    1 nothing -- its frames still hold the poison"""
    sc, osn = cube
    res, n = (40, 16), 260
    st = vrt.VoxelRenderSettings.primary_only(res)
    stc = st.to_c()
    plist = [_pose(vrt, res, "sweep", f % 13) for f in range(n)]
    exp = _expected(oracle, osn, st, plist[:13])
    pushes = (vrt._capi.Push * n)(*plist)
    shards = (vrt._capi.Shard * n)(*[vrt._capi.Shard(f % 2, 2, 16) for f in range(n)])
    out = _six_planes(vrt, engine, n, res)
    vrt._capi.check(vrt.lib().vrt_render_geometry_slots(engine.ctx, sc.handle, n, pushes, C.byref(stc), out.c, shards))
    engine.synchronize()
    got = out.bytes()
    for f in range(n):
        if f % 2 == 0:
            _same_typed(got, f, exp[f % 13], ("slots", f))
        else:
            assert all((got[k][f] == lsc.POISON).all() for k in SIX), ("slots", f)


def test_box_edits_add_and_remove_the_only_cell_under_a_span(vrt, oracle, engine):
    vol, pal = _volume(), metallic_palette(vrt)
    sky, noise = _noise_sky(256, 128, 5), vrt.synthetic.blue_noise_standin(32)
    sc = vrt.VoxelScene.from_dense(engine, vol, pal, sky=sky, noise=noise)
    res = (100, 13)
    st = vrt.VoxelRenderSettings.primary_only(res)
    pushes = [_pose(vrt, res, "sweep", f) for f in range(12)]
    try:
        for step, (lo, ids) in enumerate([((14, 14, 14), np.zeros((4, 4, 4), np.uint8)),          # remove the cube: all sky
                                          ((4, 14, 14), np.full((4, 4, 4), 9, np.uint8)),         # a cube somewhere else
                                          ((4, 14, 14), np.zeros((4, 4, 4), np.uint8))]):         # and away again
            sc.edit(lo, ids)
            x, y, z = lo
            vol[z:z + ids.shape[0], y:y + ids.shape[1], x:x + ids.shape[2]] = ids
            osn = oracle.OracleScene(vol, pal, sky=sky, noise=noise)
            exp = _expected(oracle, osn, st, pushes)
            assert any((e["hit_id"] != 0).any() for e in exp) == (step == 1)
            _check(_frames(vrt, engine, sc, st, pushes[:1], 1, SIX), exp[:1], ("edit", step, "one frame"))
            _check(_stage_batch(vrt, engine, sc, st, pushes, 1), exp, ("edit", step, "12 in the table"))
    finally:
        sc.destroy()


def test_six_table_launches_behind_a_stalled_stream(vrt, oracle, engine, cube):
    """Six launches of nine frames, each with poses of its own, enqueued behind a busy stream and synchronised once: the fifth takes
    the table ring slot of the first, and every launch the tag and verdict buffers of the launch before last, while those may not
    have started.  Every frame equals the oracle's."""
    sc, osn = cube
    res, L, n = (72, 13), 6, 9
    st = vrt.VoxelRenderSettings.primary_only(res)
    stc = st.to_c()
    plist = [_pose(vrt, res, "sweep" if (f // n) % 2 == 0 else "sky", f % 12) for f in range(L * n)]
    exp = _expected(oracle, osn, st, plist)
    outs = [_six_planes(vrt, engine, n, res) for _ in range(L)]
    pushes = [(vrt._capi.Push * n)(*plist[k * n:(k + 1) * n]) for k in range(L)]
    engine.synchronize()
    keep = _stall(engine.torch_device)
    for k in range(L):
        vrt._capi.check(vrt.lib().vrt_render_geometry_batch(engine.ctx, sc.handle, n, pushes[k], C.byref(stc), outs[k].c, None))
    engine.synchronize()
    del keep
    for k in range(L):
        got = outs[k].bytes()
        for f in range(n):
            _same_typed(got, f, exp[k * n + f], ("ring", k, f))
