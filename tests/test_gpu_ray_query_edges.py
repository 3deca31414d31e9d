"""Ray queries on the GPU at the edges of the finite-ray contract (include/vrt.h): the ray classes of ray_query_common.edge_rays, the
long volume on either side of VRT_TRAVERSAL_AUTO's switch at max_steps 1024 / 1025, axis-aligned orthographic views against a
statement in numpy, and a pick from a lattice camera position.  tests/test_ray_query_cpu.py holds the same classes against the
oracle on the host build first; this file is what the host build cannot reach -- the hand-written look-up loops.

What the look-up loops (csrc/vrt_march_fast.h: trace_df_fast over df_fast_loop / df_prim_loop) index, class by class.  The set-up forms
ONE first index, idx0 = bias + oct * stride + df_index(first mapPos) when the first mapPos is inside the volume, else the sentinel
(the 0xFF byte behind the ninth field: the lane is finished before it starts, its deltas and increments are 0).  Every later index is
either the previous one moved by incx = +-1, incy = +-pw, incz = +-pwh per step of a short run (integers, exact), or idx0 + nx +
ny * pw + nz * pwh with n = rint(side * g + c), g = dir (0 for an axis whose deltaDist is infinite) and c = -side0 * g.  A run is never
longer than the clearance read, the border has clearance 0, so the cell of every look-up is a cell the reference's loop visits: inside
the volume or in the one-voxel border, i.e. inside the padded fields; the prefetches reach one row / slice further, into df_guard.
That argument needs (a) the first mapPos to be the reference's, (b) n to be exact.
  axis1, axis2, negzero, ortho_grid, lattice_in
              a zero component has deltaDist = inf, so g = 0, c = 0 and v_mul_legacy_f32 gives inf * 0 = 0: n = 0 on that axis.  The
              other axes are ordinary: |error of n| <= (n^2 + 3n) 2^-24 < 1/16 for max_steps <= 1024 (measured 0.016 on the long
              volume).  -0.0 compares equal to 0 in fsign and its reciprocal is -inf, |.| = inf: the same.  Ties step several axes in
              one iteration; each axis' n counts its own additions.
  zero        inside: all three deltaDist are inf: g = c = 0, inc = 0 (rayStep 0): every look-up is idx0.  Outside, on the side
              where boxIntersection is defined (tmax = -inf: the test fails): first mapPos = floor(origin), outside, sentinel.  tspan is inf and the bound of the
              budget-free loop inf * 0 = NaN, which fails `bound < maxSteps`: the wave takes df_fast_loop, which counts.
  scaled      sideDist and deltaDist scale by 2^-k, g by 2^k: the products are those of the unscaled ray, bit for bit, until a factor
              leaves the normal range -- 2^+-60 times 0.3 .. 2 and distances below 2^9 stay within 2^+-80.  For k > 10 or so the
              + 0.1 of boxIntersection throws the point out of the volume: first mapPos outside (saturated on conversion), sentinel.
  far         boxIntersection's point has the origin's rounding error, up to 10^23 voxels: either the first mapPos is outside
              (saturated conversion, sentinel) or it is an ordinary start inside, and no index is formed from the origin again.
              The origin does reach one more decision: a wave enters the budget-free df_prim_loop when tspan * (|dx| + |dy| + |dz|)
              * 1.001 + 8 < max_steps for all its rays, and tspan = tmax - t0 is wrong by up to 2^-22 * 3 * |origin| steps -- more
              than the margin of 8 from about 10^7 voxels on, so that an under-bounded ray could march past its budget (in bounds:
              the loop still ends at the border).  k_query clears df_thresh for a wave that holds an origin component beyond 2^20
              (csrc/vrt_query.h, query_far_origin), where the error is below one step: far takes df_fast_loop, which counts.
  tiny        NOT launched through the look-up loops: for 2^-128 < |d| < 2^-126 deltaDist is finite (up to 2^128), g = d is
              subnormal, and side * g + c is exact only if v_mul_legacy_f32 and the compiled multiply that forms c treat subnormal
              factors alike, which the code does not show.  k_query sends a wave that holds a subnormal component through
              VRT_TRAVERSAL_DF (query_subnormal_component), whose recovery multiplies the sideDist travelled in a run: exactly 0 for
              an axis that did not step, whatever g is.
The rays the contract leaves open (ray_query_common.open_set) are in no batch here."""
import numpy as np
import pytest

from helpers import camera_push, metallic_palette
from ray_query_common import (EDGE_CLASSES, LONG_BUDGETS, LONG_DIMS, bricks_of, edge_rays, long_rays, long_volume, open_set, oracle_records,
                              ortho_grid_rays, planes_differ)
from test_gpu_ray_query import _volume

pytestmark = pytest.mark.gpu

BUDGETS = (1024, 37, 1)
N = 4096
ODD_DIMS = (37, 5, 70)


def _odd_volume():
    rng = np.random.default_rng(15)
    W, H, D = ODD_DIMS
    vol = ((rng.random((D, H, W)) < 0.01) * rng.integers(1, 256, (D, H, W))).astype(np.uint8)
    vol[D // 2:, :1, :] |= np.uint8(7)
    return vol


@pytest.fixture(scope="module")
def world(vrt, oracle, engine):
    """The 64^3 volume as a dense and as a brick scene, the 37 x 5 x 70 volume as a dense scene, 4 096 rays of every class on either
    volume, and the oracle's records of them, computed once per (volume, class, budget) and shared by the tests below."""
    pal = metallic_palette(vrt)
    vols = {"cube": _volume(), "odd": _odd_volume()}
    dims = {"cube": (64, 64, 64), "odd": ODD_DIMS}
    grid, pool = bricks_of(vols["cube"])
    scenes = {"cube": {"dense": vrt.VoxelScene.from_dense(engine, vols["cube"], pal), "brick": vrt.VoxelScene.from_bricks(engine, grid, pool, pal)},
              "odd": {"dense": vrt.VoxelScene.from_dense(engine, vols["odd"], pal)}}
    osn = {k: oracle.OracleScene(v, pal) for k, v in vols.items()}
    rays, cache = {}, {}
    for vi, v in enumerate(vols):
        for ci, cls in enumerate(EDGE_CLASSES):
            s, d = edge_rays(np.random.default_rng(7000 + 100 * vi + ci), N, dims[v], cls, vols[v])
            comp, open_rays = open_set(s, d, dims[v])
            assert not comp.any() and not open_rays.any()
            rays[(v, cls)] = (s, d)

    def expected(v, cls, ms):
        if (v, cls, ms) not in cache:
            cache[(v, cls, ms)] = oracle_records(oracle, osn[v], *rays[(v, cls)], ms)[0]
        return cache[(v, cls, ms)]

    yield {"scenes": scenes, "rays": rays, "expected": expected}
    for group in scenes.values():
        for sc in group.values():
            sc.destroy()


def _check(world, v, s, d, ms, exp, what):
    got = {}
    for kind, sc in world["scenes"][v].items():
        got[kind] = sc.trace_rays(s, d, ms)
        bad = planes_differ(got[kind], exp)
        assert bad.size == 0, (what, v, kind, ms, bad[:5], {k: a[bad[:3]] for k, a in got[kind].items()}, {k: a[bad[:3]] for k, a in exp.items()},
                               s[bad[:3]], d[bad[:3]])
        miss = exp["material"] == 0
        assert not got[kind]["pos"][miss].any() and not got[kind]["voxel"][miss].any() and not got[kind]["normal"][miss].any()
        occ = sc.occluded(s, d, ms)
        assert (occ == (exp["material"] != 0)).all(), (what, v, kind, ms, np.flatnonzero(occ != (exp["material"] != 0))[:5])
    if "brick" in got:
        assert planes_differ(got["dense"], got["brick"]).size == 0, (what, ms)


@pytest.mark.parametrize("cls", EDGE_CLASSES)
def test_class_alone_matches_oracle(world, cls):
    """4 096 rays of one class, at max_steps (1024, 37, 1), on the 64^3 volume (dense and bricks) and the 37 x 5 x 70 volume: every
    plane of vrt_trace_rays equals the oracle, a miss is 0 everywhere, vrt_occluded_rays equals material != 0, dense equals brick."""
    for v in ("cube", "odd"):
        s, d = world["rays"][(v, cls)]
        for ms in BUDGETS:
            exp = world["expected"](v, cls, ms)
            if ms == 1024:
                assert (exp["material"] != 0).any() and (exp["material"] == 0).any(), (v, cls)
            _check(world, v, s, d, ms, exp, cls)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_prefixes_of_a_class(world, n):
    """The first 1, 63, 64 and 65 rays of lattice_in: a wave with one ray, one short of full, full, and a second wave with one."""
    for v in ("cube", "odd"):
        s, d = (a[:n] for a in world["rays"][(v, "lattice_in")])
        for ms in BUDGETS:
            exp = {k: a[:n] for k, a in world["expected"](v, "lattice_in", ms).items()}
            _check(world, v, s, d, ms, exp, ("prefix", n))


def test_classes_interleaved_match_oracle(world):
    """All classes in one batch, ray i of class i % 9: a wave holds rays that finish in iteration 0 next to long ones, rays of every
    octant, and rays with a subnormal component (the wave then takes VRT_TRAVERSAL_DF) next to those without."""
    k = len(EDGE_CLASSES)
    for v in ("cube", "odd"):
        s = np.stack([world["rays"][(v, c)][0] for c in EDGE_CLASSES], axis=1).reshape(-1, 3)
        d = np.stack([world["rays"][(v, c)][1] for c in EDGE_CLASSES], axis=1).reshape(-1, 3)
        assert len(s) == k * N and (s[3] == world["rays"][(v, EDGE_CLASSES[3])][0][0]).all()
        for ms in BUDGETS:
            per = [world["expected"](v, c, ms) for c in EDGE_CLASSES]
            exp = {p: np.stack([e[p] for e in per], axis=1).reshape((k * N,) + per[0][p].shape[1:]) for p in per[0]}
            _check(world, v, np.ascontiguousarray(s), np.ascontiguousarray(d), ms, exp, "interleaved")


@pytest.mark.parametrize("mirrored", [False, True])
def test_long_volume_on_both_sides_of_the_switch(vrt, oracle, engine, mirrored):
    """The 1100 x 8 x 8 volume (mirrored: its mirror image, rays along -x) as a dense scene, 2 000 near-axis rays whose hits need 850
    .. 1100 iterations: at max_steps 1023 and 1024 the look-up loop with its position recovery at the edge of its bound, at 1025
    and 2000 VRT_TRAVERSAL_DF -- both equal the oracle, and the hits at 1025 are those at 1024 plus exactly the rays whose hit is
    the 1025th fetch."""
    pal = metallic_palette(vrt)
    vol = long_volume(mirrored)
    sc = vrt.VoxelScene.from_dense(engine, vol, pal)
    osn = oracle.OracleScene(vol, pal)
    s, d = long_rays(2000, mirrored)
    _, _, steps = oracle_records(oracle, osn, s, d, 2000, with_steps=True)
    hits = {}
    for ms in LONG_BUDGETS:
        exp, _ = oracle_records(oracle, osn, s, d, ms)
        got = sc.trace_rays(s, d, ms)
        bad = planes_differ(got, exp)
        assert bad.size == 0, (ms, bad[:5], {k: a[bad[:3]] for k, a in got.items()}, {k: a[bad[:3]] for k, a in exp.items()}, steps[bad[:5]])
        assert (sc.occluded(s, d, ms) == (exp["material"] != 0)).all(), ms
        hits[ms] = got["material"] != 0
    assert (hits[2000] & (steps >= 850) & (steps <= 1100)).mean() >= 0.5
    gained = hits[1025] & ~hits[1024]
    assert not (hits[1024] & ~hits[1025]).any() and gained.any()
    assert (gained == (hits[2000] & (steps == 1025))).all()
    sc.destroy()


def _ortho_expected(vol, o, axis, sign, ms):
    """The numpy statement: a ray along sign * e_axis from a point whose two other coordinates lie in column (floor u, floor v) hits
    the first non-zero voxel of that column in its direction of travel, within the budget (the march starts at the cell that
    boxIntersection's point, 0.1 past the face, lies in: the first cell of the column, one iteration per cell); a ray beside the
    volume misses.  Also returned: whether the hit is the column's first cell."""
    D, H, W = vol.shape
    size = (W, H, D)
    u, v = [b for b in range(3) if b != axis]
    mat = np.zeros(len(o), np.uint8); cell = np.zeros((len(o), 3), np.int32); at_once = np.zeros(len(o), bool)
    for i, p in enumerate(o):
        cu, cv = int(np.floor(p[u])), int(np.floor(p[v]))
        if not (0 <= cu < size[u] and 0 <= cv < size[v]):
            continue
        order = range(size[axis]) if sign > 0 else range(size[axis] - 1, -1, -1)
        for k, c in enumerate(order):
            if k >= ms:
                break
            idx = [0, 0, 0]; idx[axis] = c; idx[u] = cu; idx[v] = cv
            if vol[idx[2], idx[1], idx[0]] != 0:
                mat[i] = vol[idx[2], idx[1], idx[0]]; cell[i] = idx; at_once[i] = k == 0
                break
    return mat, cell, at_once


@pytest.mark.parametrize("axis,sign", [(a, s) for a in range(3) for s in (1, -1)])
def test_axis_aligned_orthographic_view(world, vrt, engine, oracle, axis, sign):
    """A 64 x 32 frame of parallel rays along one of the six axis directions, supplied as ray buffers: vrt_trace_rays equals the
    oracle, and equals the numpy statement of _ortho_expected -- material and voxel; the normal is -sign * e_axis; pos along the axis
    is the near face of the voxel hit within 1e-4 (0.2 behind it for a voxel of the column's first cell, as traceRay has it) and the two other coordinates are the origin's, bit for bit."""
    vol = _volume()
    o, d = ortho_grid_rays((64, 64, 64), axis, sign, 64, 32)
    o, d = np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)
    comp, open_rays = open_set(o, d, (64, 64, 64))
    assert not comp.any() and not open_rays.any()
    osn = oracle.OracleScene(vol, metallic_palette(vrt))
    for ms in (1024, 37):
        exp, _ = oracle_records(oracle, osn, o, d, ms)
        _check(world, "cube", o, d, ms, exp, ("ortho", axis, sign))
        got = world["scenes"]["cube"]["dense"].trace_rays(o, d, ms)
        mat, cell, at_once = _ortho_expected(vol, o, axis, sign, ms)
        hit = mat != 0
        assert hit.any() and (~hit).any()
        assert (got["material"] == mat).all() and (got["voxel"] == cell).all()
        nrm = np.zeros((len(o), 3), np.int8); nrm[hit, axis] = -sign
        assert (got["normal"] == nrm).all()
        # a hit in the column's first cell is found before the loop has stepped: traceRay then adds length(sideDist - deltaDist) =
        # |0.9 - 1| to boxIntersection's point, which lies 0.1 behind the face already (frag:122, 187-192)
        face = cell[:, axis] + (0 if sign > 0 else 1) + np.where(at_once, 0.2 * sign, 0.0)
        assert (hit & at_once).any() and (hit & ~at_once).any()
        assert np.abs(got["pos"][hit, axis] - face[hit]).max() < 1e-4
        for b in range(3):
            if b != axis:
                assert (got["pos"][hit, b].view(np.uint32) == o[hit, b].view(np.uint32)).all()


def test_pick_from_a_lattice_camera_position(vrt, engine):
    """vrt_pick_pixels on the 37 x 5 x 70 volume at a 65 x 5 frame from a camera on integer coordinates looking along +z (yaw 90, pitch
    0): the records equal the frame's hit_id / hit_voxel / position / hit_mask planes."""
    W, H = 65, 5
    vol = _odd_volume()
    sc = vrt.VoxelScene.from_dense(engine, vol, metallic_palette(vrt), sky=vrt.synthetic.sky_gradient(64, 32))
    st = vrt.VoxelRenderSettings.primary_only((W, H))
    push = camera_push(vrt, ODD_DIMS, (W, H), pos=(18.0, 2.0, -20.0), yaw=90.0, pitch=0.0)
    g = vrt.GeometryStage(engine, st, sc, debug_planes=True).record(push)
    engine.synchronize()
    g = g.numpy()
    hit_id = g["hit_id"].reshape(-1)
    assert (hit_id != 0).any() and (hit_id == 0).any()
    ys, xs = np.mgrid[0:H, 0:W]
    xy = np.stack([xs.reshape(-1), ys.reshape(-1)], axis=1).astype(np.int32)
    rec = sc.pick(push, xy, st.traceSettings.maxRaySteps)
    assert (rec["material"] == hit_id).all()
    assert (rec["pos"].view(np.uint32) == g["position"].reshape(-1, 4)[:, :3].view(np.uint32)).all()
    assert (rec["voxel"] == g["hit_voxel"].reshape(-1, 3).astype(np.int32)).all()
    mask = g["hit_mask"].reshape(-1)
    assert ((rec["normal"] != 0) == np.stack([(mask >> a) & 1 for a in range(3)], axis=1).astype(bool)).all()
    assert (rec["normal"] == np.sign(g["normal8"].reshape(-1, 4)[:, :3])).all()
    sc.destroy()
