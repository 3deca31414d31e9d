"""The miss-colour planes (csrc/vrt_miss_plane.h; k_miss_plane; the skip branch of k_primary MODE 1 in table launches) on the GPU:
a 64^3 scene with sky around it, frames of 104x40 (the right edge cuts a span; five block rows) and 96x24 (every span whole),
launches of 9 and 12 frames in the slot table.  Every plane of every frame is compared bit for bit with the same launch under
sky_plane = 0 and with the oracle; the context's read-only options say which frames loaded from a plane and how many planes were built.

  (a) all frames share one view (a dolly: the position moves, nothing else)
  (b) two views, 6 + 6 frames: both groups get planes
  (c) 11 frames of one view and one rotated frame: the odd frame runs the path without a plane
  (d) the same launch twice (the second builds nothing), then with the sky replaced: the new sky is what the frames show
  (e) sky_span = 0 with sky_plane = 1
  (f) a sharded table launch (two ranks, 16-row strips)
  (g) a view in which some sky pixels are not sure of their texel by the header's own sky_texel_fast (asserted on the CPU)
and vrt_scene_trim drops the planes."""

import numpy as np
import pytest

from helpers import camera_push, metallic_palette
from test_gpu_sky_span import ORACLE, SIX, _frames, _noise_sky, _same, _sure

pytestmark = pytest.mark.gpu

DIMS = (64, 64, 64)
SIX_ORACLE = [k for k in ORACLE if k in SIX]
SIZES = [(104, 40), (96, 24)]


def _volume():
    """a few boxes around the middle of an empty 64^3 volume: from outside, most of every frame is sky"""
    vol = np.zeros((64, 64, 64), np.uint8)
    vol[24:40, 28:36, 24:40] = 3
    vol[30:34, 36:48, 30:34] = 9
    vol[8:12, 8:12, 8:12] = 201
    return vol


def _scene(vrt, oracle, engine, sky):
    vol, pal, noise = _volume(), metallic_palette(vrt), vrt.synthetic.blue_noise_standin(32)
    return vrt.VoxelScene.from_dense(engine, vol, pal, sky=sky, noise=noise), oracle.OracleScene(vol, pal, sky=sky, noise=noise)


@pytest.fixture(scope="module")
def scene(vrt, oracle, engine):
    sc, osn = _scene(vrt, oracle, engine, _noise_sky(256, 128, 11))
    yield sc, osn
    sc.destroy()


def _dolly(vrt, res, n, yaw=90.0, pitch=0.0, first=0):
    """n frames of one view: the camera backs away and drifts sideways, its basis does not change"""
    return [camera_push(vrt, DIMS, res, (30.0 + 0.7 * f, 33.0 - 0.4 * f, -50.0 - 2.0 * f), yaw, pitch, frame=f) for f in range(first, first + n)]


def _planes_state(vrt, engine, n):
    """planes built so far, planes held, the rule's minimum group, and which plane each frame of the latest launch loaded from"""
    return (engine.option("sky_planes_built"), engine.option("sky_planes_held"), engine.option("sky_plane_min_group"),
            [engine.option(f"sky_plane_of_{f}") for f in range(n)])


def _launch(vrt, engine, sc, st, pushes, plane, span=1, shard=None):
    with engine.options(sky_plane=plane):
        got = _frames(vrt, engine, sc, st, pushes, span, SIX, shard=shard)
    return got, _planes_state(vrt, engine, len(pushes))


def _expected(oracle, osn, st, pushes):
    return [oracle.render(osn, p, oracle.params_from(st.to_c()), planes=ORACLE, nthreads=8) for p in pushes]


def _check(on, off, exp, what, rows=None):
    for f in range(len(on)):
        _same(on[f], off[f], SIX, what + (f, "sky_plane = 0"), rows=rows)
        _same(on[f], exp[f], SIX_ORACLE, what + (f, "oracle"), rows=rows)
        assert not (on[f]["motion"] if rows is None else on[f]["motion"][rows]).any(), what + (f,)


@pytest.mark.parametrize("n", [9, 12])
@pytest.mark.parametrize("res", SIZES)
def test_a_one_view(vrt, oracle, engine, scene, res, n):
    sc, osn = scene
    sc.trim()
    st = vrt.VoxelRenderSettings.primary_only(res)
    pushes = _dolly(vrt, res, n)
    exp = _expected(oracle, osn, st, pushes)
    miss = np.stack([e["hit_id"].reshape(res[1], res[0]) == 0 for e in exp])
    assert miss.mean() > 0.5 and not miss.all()                       # mostly sky, and something to trace
    b0 = _planes_state(vrt, engine, 0)[0]
    on, (b1, held, G, which) = _launch(vrt, engine, sc, st, pushes, 1)
    assert n >= G and b1 == b0 + 1 and held == 1
    assert which[0] != 0 and which == [which[0]] * n
    off, (b2, _, _, which_off) = _launch(vrt, engine, sc, st, pushes, 0)
    assert b2 == b1 and which_off == [0] * n
    _check(on, off, exp, ("a", res, n))


def test_b_two_views_of_six_frames(vrt, oracle, engine, scene):
    sc, osn = scene
    sc.trim()
    for res in SIZES:
        st = vrt.VoxelRenderSettings.primary_only(res)
        pushes = _dolly(vrt, res, 6) + _dolly(vrt, res, 6, yaw=97.0, pitch=4.0, first=6)
        exp = _expected(oracle, osn, st, pushes)
        b0 = _planes_state(vrt, engine, 0)[0]
        on, (b1, held, G, which) = _launch(vrt, engine, sc, st, pushes, 1)
        assert G <= 6 and b1 == b0 + 2
        assert which[:6] == [which[0]] * 6 and which[6:] == [which[6]] * 6 and 0 not in which and which[0] != which[6]
        off, _ = _launch(vrt, engine, sc, st, pushes, 0)
        _check(on, off, exp, ("b", res))


def test_c_eleven_frames_and_a_rotated_one(vrt, oracle, engine, scene):
    sc, osn = scene
    sc.trim()
    for res in SIZES:
        st = vrt.VoxelRenderSettings.primary_only(res)
        pushes = _dolly(vrt, res, 12)
        pushes[7] = camera_push(vrt, DIMS, res, (30.0, 33.0, -60.0), 84.0, -3.0, frame=7)
        exp = _expected(oracle, osn, st, pushes)
        on, (_, _, _, which) = _launch(vrt, engine, sc, st, pushes, 1)
        assert which[7] == 0 and all(w == which[0] != 0 for i, w in enumerate(which) if i != 7)
        off, _ = _launch(vrt, engine, sc, st, pushes, 0)
        _check(on, off, exp, ("c", res))


def test_d_twice_and_then_another_sky(vrt, oracle, engine):
    sky_a, sky_b = _noise_sky(256, 128, 11), _noise_sky(128, 64, 12)
    sc, osn = _scene(vrt, oracle, engine, sky_a)
    try:
        res = SIZES[0]
        st = vrt.VoxelRenderSettings.primary_only(res)
        pushes = _dolly(vrt, res, 9)
        exp = _expected(oracle, osn, st, pushes)
        on, (b1, _, _, which1) = _launch(vrt, engine, sc, st, pushes, 1)
        again, (b2, _, _, which2) = _launch(vrt, engine, sc, st, pushes, 1)
        assert b2 == b1 and which2 == which1 and 0 not in which1   # the second launch found its plane
        off, _ = _launch(vrt, engine, sc, st, pushes, 0)
        _check(on, off, exp, ("d", "first"))
        _check(again, off, exp, ("d", "second"))
        sc.set_sky(sky_b)
        osn_b = oracle.OracleScene(_volume(), metallic_palette(vrt), sky=sky_b, noise=vrt.synthetic.blue_noise_standin(32))
        exp_b = _expected(oracle, osn_b, st, pushes)
        assert any((exp_b[f]["color8"] != exp[f]["color8"]).any() for f in range(9))
        new, (b3, _, _, which3) = _launch(vrt, engine, sc, st, pushes, 1)
        assert b3 == b2 + 1 and 0 not in which3                      # a plane of the new sky, not the old one
        off_b, _ = _launch(vrt, engine, sc, st, pushes, 0)
        _check(new, off_b, exp_b, ("d", "new sky"))
    finally:
        sc.destroy()


def test_e_without_the_span_path(vrt, oracle, engine, scene):
    sc, osn = scene
    for res in SIZES:
        st = vrt.VoxelRenderSettings.primary_only(res)
        pushes = _dolly(vrt, res, 9)
        exp = _expected(oracle, osn, st, pushes)
        on, (_, _, _, which) = _launch(vrt, engine, sc, st, pushes, 1, span=0)
        assert 0 not in which
        off, _ = _launch(vrt, engine, sc, st, pushes, 0, span=0)
        _check(on, off, exp, ("e", res))


def test_f_two_shards(vrt, oracle, engine, scene):
    sc, osn = scene
    res = SIZES[0]
    st = vrt.VoxelRenderSettings.primary_only(res)
    pushes = _dolly(vrt, res, 12)
    exp = _expected(oracle, osn, st, pushes)
    owned = {0: [slice(0, 16), slice(32, 40)], 1: [slice(16, 32)]}
    for rank in (0, 1):
        shard = vrt._capi.Shard(rank, 2, 16)
        on, (_, _, _, which) = _launch(vrt, engine, sc, st, pushes, 1, shard=shard)
        assert 0 not in which
        off, _ = _launch(vrt, engine, sc, st, pushes, 0, shard=shard)
        for rows in owned[rank]:
            _check(on, off, exp, ("f", rank, rows.start), rows=rows)


def test_g_a_view_with_unsure_texels(vrt, oracle, engine):
    """a 97 x 41 sky and a camera that looks steeply up: some sky pixels lie within sky_texel_fast's bound of a texel edge.  The
    plane holds the long path's word for them, which is what their wave stores without a plane."""
    sw, sh = 97, 41
    sc, osn = _scene(vrt, oracle, engine, _noise_sky(sw, sh, 8))
    try:
        for res in SIZES:
            st = vrt.VoxelRenderSettings.primary_only(res)
            pushes = [camera_push(vrt, DIMS, res, (30.0 + f, -90.0 - 3.0 * f, 20.0), 45.0, 70.0, frame=f) for f in range(9)]
            exp = _expected(oracle, osn, st, pushes)
            miss = exp[0]["hit_id"].reshape(res[1], res[0]) == 0
            sure = _sure(pushes[0], sw, sh)
            assert (miss & ~sure).any() and (miss & sure).any(), (res, int((miss & ~sure).sum()))
            on, (_, _, _, which) = _launch(vrt, engine, sc, st, pushes, 1)
            assert 0 not in which
            off, _ = _launch(vrt, engine, sc, st, pushes, 0)
            _check(on, off, exp, ("g", res))
    finally:
        sc.destroy()


def test_trim_drops_the_planes(vrt, engine, scene):
    sc, _ = scene
    res = SIZES[1]
    st = vrt.VoxelRenderSettings.primary_only(res)
    _launch(vrt, engine, sc, st, _dolly(vrt, res, 9), 1)
    assert _planes_state(vrt, engine, 0)[1] >= 1
    sc.trim()
    assert _planes_state(vrt, engine, 0)[1] == 0
