"""K1's shorter preamble (one four-word tag fetch, one compare chain, one rectangle test: csrc/vrt_span.h span_verdict /
span_decide) on the GPU, at the smallest shapes at which they can go
wrong: a 100x44 frame (whole spans at x = 0, 32, 64, a span cut by the right edge at 96, rows that are no multiple of 8) and a
32x8 frame (exactly one span), the six-target launch with one frame and with three frames of a batch, over a scene of a few
cubes so that a launch holds all-sky spans, spans with one to three tagged blocks and traced waves.  Every frame equals, bit for
bit on every plane, the oracle's, the same launch with sky_span = 0 and the launch without tags.  Camera A looks along an axis
from outside; camera D is pitched up 35 degrees so that some sky waves have lanes more than 30 degrees from the horizon (the
upper range of the sky texel's asin) and some have none -- asserted from the ray directions.  Camera B looks along a face diagonal of the
cubes, so that rays whose x and z steps tie hit edges (2-bit masks, asserted); camera C sits inside a solid voxel, so that every
hit is rule A's (mask 0, ncode 0xFFFFFFFF, asserted).  Corner hits (3-bit masks, asserted) need a pixel whose ray is an exact
space diagonal; at even widths and heights no pixel centre lies on the optical axis, so they have a case of their own on a
101x45 frame (test_corner_hits_on_an_odd_frame).  Three launches per case: one frame, three
frames through GeometryStage.prepare_batch (slots in the kernel arguments) and twelve through it (slots in the table)."""
import numpy as np
import pytest

from helpers import camera_push, metallic_palette
from test_gpu_sky_span import ORACLE, SIX, _frames, _noise_sky, _ray_v, _same, _span_kinds

pytestmark = pytest.mark.gpu

# position, yaw, pitch (the scene is 32^3)
CAMS = {"A": ((16.0, 16.0, -70.0), 90.0, 0.0),        # axis-aligned, outside: one-axis hits only
        "B": ((-4.0, 16.0, -4.0), 45.0, 0.0),          # along a face diagonal: rays whose x and z steps tie, edge masks
        "C": ((23.5, 14.5, 20.5), 90.0, 0.0),          # inside a solid voxel: every ray ends where it starts, rule A
        "D": ((16.0, 4.0, -70.0), 90.0, 35.0)}         # pitched up 35 degrees
CAM_A, CAM_D = CAMS["A"], CAMS["D"]


def _push(vrt, res, cam, frame, dx=0.0):
    (x, y, z), yaw, pitch = cam
    return camera_push(vrt, (32, 32, 32), res, (x + dx, y, z), yaw, pitch, frame=frame)


def _big_blocks(push, hit_id):
    """of the 8x8 blocks of the frame without a hit: how many hold a ray with |vy| / |v| > 0.5, and how many hold none"""
    v = _ray_v(push).astype(np.float64)
    a = np.abs(v[..., 1]) / np.sqrt((v * v).sum(-1))
    H, W = a.shape
    hit = hit_id.reshape(H, W) != 0
    some = none = 0
    for y in range(0, H, 8):
        for x in range(0, W, 8):
            if hit[y:y + 8, x:x + 8].any():
                continue
            b = a[y:y + 8, x:x + 8]
            # (a margin around the threshold: the kernel's float ratio may differ in the last bits)
            some += bool((b > 0.501).any())
            none += bool((b < 0.499).all())
    return some, none


@pytest.fixture(scope="module")
def cubes(vrt, oracle, engine):
    vol = vrt.synthetic.floating_cubes(32, seed=5, count=12)
    pal = metallic_palette(vrt)
    sky, noise = _noise_sky(512, 256, 21), vrt.synthetic.blue_noise_standin(32)
    sc = vrt.VoxelScene.from_dense(engine, vol, pal, sky=sky, noise=noise)
    yield sc, oracle.OracleScene(vol, pal, sky=sky, noise=noise)
    sc.destroy()


def _popcount(m):
    m = m.astype(np.uint32)
    return (m & 1) + ((m >> 1) & 1) + ((m >> 2) & 1)


def _stage_batch(vrt, engine, sc, st, pushes, span, tile_tags=1):
    """the frames of one launch through GeometryStage.prepare_batch (the six targets): more than 8 frames travel in the slot table"""
    launch = vrt.GeometryStage(engine, st, sc).prepare_batch(len(pushes))
    with engine.options(sky_span=span, tile_tags=tile_tags):
        gbs = launch(pushes)
        engine.synchronize()
    return [{k: np.array(v, copy=True) for k, v in g.numpy().items()} for g in gbs]


def _compare_launch_forms(vrt, oracle, engine, sc, st, pushes, exp, what):
    """one frame (vrt_render_geometry_batch, n = 1), 3 frames through prepare_batch (slots in the kernel arguments) and all of them
    (more than VRT_MAX_BATCH = 8: slots in the table): each against the oracle, sky_span = 0 and the launch without tags"""
    six_oracle = [k for k in ORACLE if k in SIX]
    runs = {"one frame": lambda span, tags: _frames(vrt, engine, sc, st, pushes[:1], span, SIX, tile_tags=tags),
            "3 in the arguments": lambda span, tags: _stage_batch(vrt, engine, sc, st, pushes[:3], span, tags),
            "12 in the table": lambda span, tags: _stage_batch(vrt, engine, sc, st, pushes, span, tags)}
    for name, run in runs.items():
        on, off, bare = run(1, 1), run(0, 1), run(1, 0)
        for f in range(len(on)):
            w = what + (name, f)
            _same(on[f], exp[f], six_oracle, w + ("oracle",))
            _same(on[f], off[f], SIX, w + ("sky_span = 0",))
            _same(on[f], bare[f], SIX, w + ("without tags",))
            assert not on[f]["motion"].any(), w


@pytest.mark.parametrize("cam", ["A", "B", "C", "D"])
@pytest.mark.parametrize("res", [(100, 44), (32, 8)])
def test_one_frame_and_batches_through_arguments_and_table(vrt, oracle, engine, cubes, res, cam):
    """one frame (vrt_render_geometry_batch, n = 1), 3 frames through prepare_batch (slots in the kernel arguments) and 12 frames
    through prepare_batch (more than VRT_MAX_BATCH = 8: slots in the table, the form the bench line runs)"""
    sc, osn = cubes
    st = vrt.VoxelRenderSettings.primary_only(res)
    pushes = [_push(vrt, res, CAMS[cam], f, dx=(0.25 if cam == "C" else 1.5) * (f % 3)) for f in range(12)]
    exp = [oracle.render(osn, p, oracle.params_from(st.to_c()), planes=ORACLE + ["hit_mask"], nthreads=8) for p in pushes[:3]]
    exp = exp + [exp[f % 3] for f in range(3, 12)]             # (the poses repeat with period 3; the frame number is not used by primary rays)
    hit, bits = exp[0]["hit_id"].reshape(-1) != 0, _popcount(exp[0]["hit_mask"].reshape(-1))
    if res == (100, 44):
        if cam in ("A", "B", "D"):
            all_miss, mixed, partial = _span_kinds(exp[0]["hit_id"])
            assert all_miss >= 1 and mixed >= 1 and partial >= 1, (all_miss, mixed, partial)
        if cam == "A":
            assert hit.any() and (bits[hit] == 1).all()                     # one-axis hits only
        if cam == "B":
            assert (hit & (bits == 2)).sum() >= 2                           # edge masks (corner masks: test_corner_hits_on_an_odd_frame)
        if cam == "C":
            assert (hit & (bits == 0)).sum() >= 64                          # rule A: ncode == 0xFFFFFFFF
        if cam == "D":
            some, none = _big_blocks(pushes[0], exp[0]["hit_id"])
            assert some >= 4 and none >= 4, (some, none)
    _compare_launch_forms(vrt, oracle, engine, sc, st, pushes, exp, (res, cam))


def test_corner_hits_on_an_odd_frame(vrt, oracle, engine, cubes):
    """Camera B': on the space diagonal through the corner of a cube, looking along (1, 1, 1) exactly (cam_dir set by hand: its
    three components are the same bits), in a 101x45 frame, whose centre pixel lies on the optical axis: that ray starts at equal
    fractions of a voxel in x, y and z and every one of its steps is a three-way tie, so it enters the cube through the corner --
    a 3-bit mask; its neighbours hit edges (2-bit masks)."""
    sc, osn = cubes
    res = (101, 45)
    st = vrt.VoxelRenderSettings.primary_only(res)
    corner, back = (6, 12, 2), 30                                           # the cube's lowest corner; nothing lies on the diagonal before it
    pos = tuple(c - back + 0.5 for c in corner)
    pushes = []
    for f in range(12):
        p = camera_push(vrt, (32, 32, 32), res, pos, 45.0, 35.264389682754654, frame=f)
        for a in range(3):
            p.cam_dir[a] = 1.0
        pushes.append(p)
    e = oracle.render(osn, pushes[0], oracle.params_from(st.to_c()), planes=ORACLE + ["hit_mask"], nthreads=8)
    hit, bits = e["hit_id"].reshape(-1) != 0, _popcount(e["hit_mask"].reshape(-1))
    assert (hit & (bits == 3)).sum() >= 1 and (hit & (bits == 2)).sum() >= 2 and (hit & (bits == 1)).sum() >= 64
    all_miss, mixed, partial = _span_kinds(e["hit_id"])
    assert all_miss >= 1 and mixed >= 1, (all_miss, mixed, partial)
    _compare_launch_forms(vrt, oracle, engine, sc, st, pushes, [e] * 12, (res, "B'"))
