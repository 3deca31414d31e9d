"""Ray segments on the GPU (vrt_trace_segments, vrt_occluded_segments; csrc/vrt_query_seg.hip): every plane and t against
tests/segment_reference.py -- held to the oracle's vo_trace_ray first -- bit for bit, on dense scenes through the look-up loop and
through VRT_TRAVERSAL_DF and on brick scenes; batch edges and absent planes; the wave budget against the same call without it;
scene edits; the three kinds of stream; line of sight through the Python mirror."""
import ctypes as C
import itertools

import numpy as np
import pytest

import segment_common as SC
import segment_reference as SR
import stream_common as sc
from helpers import metallic_palette
from ray_query_common import bricks_of, edge_rays
from ray_query_common import planes_differ as rays_differ

pytestmark = pytest.mark.gpu
GPU_BUDGETS = (512, 37, 1, 1500)               # 1500: past the look-up loop's 1024, the dense scene takes VRT_TRAVERSAL_DF
PLANES = {"material": (np.uint8, 1), "pos": (np.float32, 3), "voxel": (np.int32, 3), "normal": (np.int8, 3), "t": (np.float32, 1)}
TAIL = 64                                       # sentinel bytes behind every plane


@pytest.fixture(scope="module")
def worlds(vrt, oracle, engine):
    """world(i): volume i of the CPU test as a dense and as a brick scene, with its rays, limits and expected records for every
    budget -- built when first asked for, once."""
    built = {}

    def get(i):
        if i not in built:
            case = SC.segment_case(oracle, *SC.VOLUMES[i], budgets=GPU_BUDGETS)
            pal = metallic_palette(vrt)
            case["dense"] = vrt.VoxelScene.from_dense(engine, case["vol"], pal)
            grid, pool = bricks_of(case["vol"])
            case["brick"] = vrt.VoxelScene.from_bricks(engine, grid, pool, pal)
            built[i] = case
        return built[i]

    yield get
    for case in built.values():
        case["dense"].destroy(); case["brick"].destroy()


@pytest.fixture(params=range(len(SC.VOLUMES)), ids=["x".join(str(d) for d in v[1]) for v in SC.VOLUMES])
def world(request, worlds):
    return worlds(request.param)


def raw_segments(vrt, engine, scene, o, d, tm, max_steps, planes, anyhit=False):
    """The C call itself on buffers with TAIL sentinel bytes behind every plane; planes that are not asked for are passed as NULL.
    Returns {plane: array} (any-hit: {"occluded": array}) after checking that no sentinel changed."""
    import torch
    dev = engine.torch_device
    n = len(o)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    do, dd, dt = to(o), to(d), to(tm)
    names = ("occluded",) if anyhit else tuple(planes)
    buf = {}
    for k in names:
        dtp, cols = (np.uint8, 1) if k == "occluded" else PLANES[k]
        buf[k] = torch.full((n * cols * np.dtype(dtp).itemsize + TAIL,), 0xA5, dtype=torch.uint8, device=dev)
    ptr = lambda k: C.c_void_p(buf[k].data_ptr()) if k in buf else None
    lib = vrt.lib()
    if anyhit:
        rc = lib.vrt_occluded_segments(engine.ctx, scene.handle, n, C.c_void_p(do.data_ptr()), C.c_void_p(dd.data_ptr()), C.c_void_p(dt.data_ptr()),
                                       max_steps, ptr("occluded"))
    else:
        rec = [k for k in names if k != "t"]
        hits = vrt._capi.RayHits(**{k: ptr(k) for k in rec})
        rc = lib.vrt_trace_segments(engine.ctx, scene.handle, n, C.c_void_p(do.data_ptr()), C.c_void_p(dd.data_ptr()), C.c_void_p(dt.data_ptr()),
                                    max_steps, C.byref(hits) if rec else None, ptr("t"))
    assert rc == 0, lib.vrt_last_error().decode()
    engine.synchronize()
    out = {}
    for k in names:
        dtp, cols = (np.uint8, 1) if k == "occluded" else PLANES[k]
        raw = buf[k].cpu().numpy()
        assert (raw[len(raw) - TAIL:] == 0xA5).all(), (k, "bytes behind the plane were written")
        a = raw[:len(raw) - TAIL].view(dtp)
        out[k] = a.reshape(n, cols) if cols > 1 else a
    return out


def _scenes(world):
    """(name, scene, budgets): the look-up loop, VRT_TRAVERSAL_DF and the brick march"""
    return (("fast", world["dense"], (512, 37, 1)), ("df", world["dense"], (1500,)), ("brick", world["brick"], (512, 37, 1)))


def test_records_match_reference(world):
    """The CPU test's volumes, rays and limits: all planes plus t equal the reference bit for bit and occluded equals its kept hits,
    through the look-up loop, VRT_TRAVERSAL_DF (max_steps 1500) and the brick march; with t_max = +inf every plane equals
    vrt_trace_rays and vrt_occluded_rays of the same call."""
    s, d, tm = world["starts"], world["dirs"], world["t_max"]
    inf = np.full(len(s), np.inf, np.float32)
    for name, scene, budgets in _scenes(world):
        for ms in budgets:
            exp = world["exp"][ms]
            got = scene.trace_segments(s, d, tm, ms)
            bad = SC.planes_differ(got, exp)
            assert bad.size == 0, (name, ms, bad[:5], {k: v[bad[:3]] for k, v in got.items()}, {k: exp[k][bad[:3]] for k in got}, s[bad[:3]], d[bad[:3]], tm[bad[:3]])
            occ = scene.occluded(s, d, ms, t_max=tm)
            assert occ.dtype == np.uint8 and (occ == exp["occluded"]).all(), (name, ms, np.flatnonzero(occ != exp["occluded"])[:5])
            open_ended = scene.trace_segments(s, d, inf, ms)
            assert rays_differ(open_ended, scene.trace_rays(s, d, ms)).size == 0, (name, ms)
            assert (open_ended["t"] == world["ref"][ms]["t"]).all()
            assert (scene.occluded(s, d, ms, t_max=inf) == scene.occluded(s, d, ms)).all(), (name, ms)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 5000])
def test_batch_sizes_and_absent_planes(vrt, engine, worlds, n):
    """n rays of the 64^3 volume (the batch edges do not depend on the volume) with sentinel bytes behind every plane: nothing is
    written past ray n - 1; every plane alone (the others NULL), t_hit alone with out == NULL, and all together give the same content."""
    world = worlds(1)
    s, d, tm = world["starts"][:n], world["dirs"][:n], world["t_max"][:n]
    for name, scene, budgets in _scenes(world):
        ms = budgets[0]
        exp = {k: v[:n] for k, v in world["exp"][ms].items()}
        got = raw_segments(vrt, engine, scene, s, d, tm, ms, tuple(PLANES))
        assert SC.planes_differ(got, exp).size == 0, (name, n)
        for k in PLANES:
            one = raw_segments(vrt, engine, scene, s, d, tm, ms, (k,))
            assert list(one) == [k] and SC.planes_differ(one, exp, (k,)).size == 0, (name, n, k)
        occ = raw_segments(vrt, engine, scene, s, d, tm, ms, (), anyhit=True)["occluded"]
        assert (occ == exp["occluded"]).all(), (name, n)


def _budget_batch(world, oracle):
    """Waves built for the wave budget, from the volume's own rays: 20 waves of one +inf lane beside 63 short limits (two voxels, or
    t_hit exactly), 20 waves of short limits only, 10 waves with every fifth limit NaN, 10 waves with every seventh ray replaced by one
    from 10^4 .. 10^30 voxels away (ray_query_common.edge_rays, "far").  The reference is held to the oracle for the rays added."""
    rng = np.random.default_rng(77)
    n = 64 * 60
    s, d = world["starts"][:n].copy(), world["dirs"][:n].copy()
    fs, fd = edge_rays(rng, n, world["dims"], "far", world["vol"])
    far = np.zeros(n, bool); far[64 * 50::7] = True
    s[far], d[far] = fs[far], fd[far]
    ref = SR.trace(world["vol"], s, d, 512)
    osn = oracle.OracleScene(world["vol"], np.zeros((256, 5), np.float32))
    bad = SR.differs_from_oracle({k: v[far] for k, v in ref.items()}, SR.oracle_trace(oracle, osn, s[far], d[far], 512))
    assert bad.size == 0 and (ref["material"][far] != 0).any()
    hit = ref["material"] != 0
    with np.errstate(divide="ignore"):
        two_voxels = (np.float32(2.0) / np.linalg.norm(d, axis=1)).astype(np.float32)
    short = np.where(hit & (rng.random(n) < 0.5), ref["t"], two_voxels).astype(np.float32)
    tm = short.copy()
    tm[0:64 * 20:64] = np.inf
    drawn = world["t_max"][:n]
    tm[64 * 40:64 * 50] = drawn[64 * 40:64 * 50]; tm[64 * 40:64 * 50:5] = np.nan
    tm[64 * 50:] = np.where(rng.random(64 * 10) < 0.5, ref["t"][64 * 50:], np.inf)
    # (as many hits whose limit is t_hit exactly as the issue asks of that class elsewhere: the bound has to cover each of them)
    assert (hit & (tm == ref["t"])).sum() >= 100 and np.isnan(tm).any() and np.isinf(tm).any()
    return s, d, tm, SR.segment_records(ref, tm)


@pytest.mark.parametrize("which", [0, 1], ids=["40x32x56", "64x64x64"])
def test_wave_budget_changes_no_result(vrt, oracle, engine, worlds, which):
    """segment_budget 1 and 0, each with thresh_runs 1 and 0: identical records, equal to the reference, on waves that mix one
    unlimited lane with 63 short segments, waves of short segments only, NaN limits and far origins -- on the two volumes large
    enough for segments much shorter than their rays.  What this cannot show is that the budget is applied at all: the results are
    the same either way by design.  That it is applied shows in profiles/segment_times.json alone; that the bound is tight enough
    to matter and never too tight is tests/test_segments_cpu.py's (own_budget, the exact-t_hit limits)."""
    world = worlds(which)
    s, d, tm, exp = _budget_batch(world, oracle)
    for name, scene, _ in _scenes(world):
        ms = 1500 if name == "df" else 512
        assert ms == 512 or (SR.trace(world["vol"], s, d, ms)["material"] == SR.trace(world["vol"], s, d, 512)["material"]).all()
        for budget, thresh in itertools.product((1, 0), (1, 0)):
            with engine.options(segment_budget=budget, thresh_runs=thresh):
                got = scene.trace_segments(s, d, tm, ms)
                occ = scene.occluded(s, d, ms, t_max=tm)
            bad = SC.planes_differ(got, exp)
            assert bad.size == 0, (name, budget, thresh, bad[:5], {k: v[bad[:3]] for k, v in got.items()}, {k: exp[k][bad[:3]] for k in got}, tm[bad[:3]])
            assert (occ == exp["occluded"]).all(), (name, budget, thresh)


@pytest.mark.parametrize("kind", ["dense", "brick"])
def test_segments_see_scene_edits(vrt, oracle, engine, kind):
    """After vrt_scene_fill_box on a dense and on a reserved brick scene a segment query sees the new volume: a wall filled across
    the rays' way, then carved again."""
    seed, dims, fill = SC.VOLUMES[0]
    vol = SC.make_volume(seed, dims, fill).copy()
    pal = metallic_palette(vrt)
    if kind == "dense":
        scene = vrt.VoxelScene.from_dense(engine, vol, pal)
    else:
        grid, pool = bricks_of(vol)
        scene = vrt.VoxelScene.from_bricks(engine, grid, pool, pal)
        scene.reserve_bricks(len(pool) + 64)
    from ray_query_common import query_rays
    s, d = query_rays(np.random.default_rng(5), 1000, dims)

    def agree():
        ref = SR.trace(vol, s, d, 512)
        osn = oracle.OracleScene(vol, np.zeros((256, 5), np.float32))
        assert SR.differs_from_oracle(ref, SR.oracle_trace(oracle, osn, s, d, 512)).size == 0
        tm = np.where(np.arange(len(s)) % 3 == 0, np.float32(np.inf), np.where(np.arange(len(s)) % 3 == 1, ref["t"], np.float32(0.5) * ref["t"])).astype(np.float32)
        exp = SR.segment_records(ref, tm)
        got = scene.trace_segments(s, d, tm, 512)
        bad = SC.planes_differ(got, exp)
        assert bad.size == 0, (kind, bad[:5])
        assert (scene.occluded(s, d, 512, t_max=tm) == exp["occluded"]).all()
        return exp

    first = agree()
    scene.fill((16, 8, 8), (8, 16, 24), 9)                    # bricks that were empty become occupied
    vol[8:32, 8:24, 16:24] = 9
    mid = agree()
    assert (mid["material"] != first["material"]).any() and (mid["material"] == 9).any()
    scene.fill((16, 8, 8), (8, 16, 24), 0)
    vol[8:32, 8:24, 16:24] = 0
    last = agree()
    assert (last["material"] != mid["material"]).any()        # (not `first` again: the carve also took what stood in the box before)
    scene.destroy()


@pytest.mark.parametrize("kind", sc.KINDS)
def test_streams_behind_a_busy_device(vrt, oracle, kind):
    """Both calls on the HIP null stream, the context's own stream and a side stream of the caller: a stall of
    tests/stream_common.py's size is enqueued, then -- with no synchronise by the caller -- vrt_trace_segments and
    vrt_occluded_segments; one vrt_ctx_synchronize, then every output against the reference.  Run once."""
    import torch
    seed, dims, fill = SC.VOLUMES[2]
    vol = SC.make_volume(seed, dims, fill)
    from ray_query_common import query_rays
    s, d = query_rays(np.random.default_rng(9), 1000, dims)
    ref = SR.trace(vol, s, d, 512)
    osn = oracle.OracleScene(vol, np.zeros((256, 5), np.float32))
    assert SR.differs_from_oracle(ref, SR.oracle_trace(oracle, osn, s, d, 512)).size == 0
    tm = np.where(np.arange(len(s)) % 2 == 0, ref["t"], np.float32(0.5) * ref["t"]).astype(np.float32)
    exp = SR.segment_records(ref, tm)
    assert exp["occluded"].any() and not exp["occluded"].all()
    side = torch.cuda.Stream() if kind == "side" else None
    with torch.cuda.stream(side if side is not None else torch.cuda.default_stream()):
        engine = vrt.Engine(0, use_torch_stream=kind != "own")
        dev = engine.torch_device
        lib, cap = vrt.lib(), vrt._capi
        scene = vrt.VoxelScene.from_dense(engine, vol, metallic_palette(vrt))
        n = len(s)
        ds, dd, dt = (torch.from_numpy(a).to(dev) for a in (s, d, tm))
        out = {k: torch.full((n, c) if c > 1 else (n,), 0x5A, dtype={np.uint8: torch.uint8, np.float32: torch.float32, np.int32: torch.int32, np.int8: torch.int8}[t], device=dev)
               for k, (t, c) in PLANES.items()}
        occ = torch.full((n,), 0x5A, dtype=torch.uint8, device=dev)
        hits = cap.RayHits(**{k: C.c_void_p(out[k].data_ptr()) for k in ("material", "pos", "voxel", "normal")})
        stall_t, stall_p = None, C.c_void_p()
        if kind == "own":
            cap.check(lib.vrt_device_alloc(engine.ctx, sc.STALL_BYTES, C.byref(stall_p)))
        else:
            stall_t = torch.zeros(sc.STALL_BYTES // 4, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        for k in range(sc.STALL_PASSES):                                 # the stall
            if kind == "own":
                cap.check(lib.vrt_memset(engine.ctx, stall_p, k, sc.STALL_BYTES))
            else:
                stall_t.add_(1.0)
        ptr = lambda t: C.c_void_p(t.data_ptr())
        cap.check(lib.vrt_trace_segments(engine.ctx, scene.handle, n, ptr(ds), ptr(dd), ptr(dt), 512, C.byref(hits), ptr(out["t"])))
        cap.check(lib.vrt_occluded_segments(engine.ctx, scene.handle, n, ptr(ds), ptr(dd), ptr(dt), 512, ptr(occ)))
        engine.synchronize()                                             # once
        if kind == "own":
            torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in out.items()}
        assert SC.planes_differ(got, exp).size == 0, kind
        assert (occ.cpu().numpy() == exp["occluded"]).all(), kind
        if kind == "own":
            lib.vrt_device_free(engine.ctx, stall_p)
        scene.destroy(); engine.destroy()


def test_cpp_host_segments(vrt, engine, tmp_path):
    """vrt_app --rays / --hits --segments on a .vox fixture (7 floats per ray in, 32 bytes per record out) writes the records
    VoxelScene.trace_segments returns."""
    import os
    import subprocess
    from ray_query_common import query_rays
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    app = os.path.join(root, "voxel-raytracing_amd", "host", "vrt_app")
    assert os.path.exists(app), "build with __graft_entry__.build()"
    path = os.path.join(root, "tests", "golden", "vox_multi.vox")
    scene = vrt.VoxelScene(engine, path)
    s, d = query_rays(np.random.default_rng(21), 3001, (scene.width, scene.height, scene.depth))
    open_ended = scene.trace_segments(s, d, np.inf, 200)
    tm = np.where(np.arange(len(s)) % 2 == 0, open_ended["t"], np.float32(0.5) * open_ended["t"]).astype(np.float32)
    rec = scene.trace_segments(s, d, tm, 200)
    assert (rec["material"] != 0).any() and ((rec["material"] == 0) & (open_ended["material"] != 0)).any()
    rays, hits = tmp_path / "rays.f32", tmp_path / "hits.bin"
    np.concatenate([s, d, tm[:, None]], axis=1).astype("<f4").tofile(rays)
    r = subprocess.run([app, "--vox", path, "--rays", str(rays), "--hits", str(hits), "--ray-steps", "200", "--segments"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    dt = np.dtype([("material", "u1"), ("pos", "<f4", 3), ("voxel", "<i4", 3), ("normal", "i1", 3), ("t", "<f4")])
    assert dt.itemsize == 32
    got = np.fromfile(hits, dtype=dt)
    assert len(got) == 3001
    assert SC.planes_differ({k: np.ascontiguousarray(got[k]) for k in PLANES}, rec).size == 0
    scene.destroy()


def test_visible_through_the_python_mirror(vrt, engine):
    """VoxelScene.visible on a scene with one wall (x in 16 .. 17 of 32^3): pairs on the same side see each other, pairs across the
    wall do not, and a b one voxel short of the wall is visible -- from inside the volume and from outside it."""
    import torch
    vol = np.zeros((32, 32, 32), np.uint8)
    vol[:, :, 16:18] = 3
    scene = vrt.VoxelScene.from_dense(engine, vol, metallic_palette(vrt))
    rng = np.random.default_rng(3)
    n = 300
    yz = lambda: rng.uniform(1.0, 31.0, (n, 2))
    left = lambda lo, hi: np.concatenate([rng.uniform(lo, hi, (n, 1)), yz()], axis=1).astype(np.float32)
    a = left(1.0, 14.0)
    assert scene.visible(a, left(1.0, 14.0)).all()                          # the same side
    assert scene.visible(left(19.0, 31.0), left(19.0, 31.0)).all()
    assert not scene.visible(a, left(19.0, 31.0)).any()                     # across the wall
    assert not scene.visible(left(19.0, 31.0), a).any()
    b = left(15.0, 15.0)                                                    # one voxel short of the wall (x = 15, the wall starts at 16)
    assert scene.visible(a, b).all()
    inside_wall = left(16.5, 17.5)
    assert not scene.visible(a, inside_wall).any()                          # b inside the wall: its own voxel is between
    outside = left(-20.0, -5.0)                                             # a outside the volume
    assert scene.visible(outside, b).all() and not scene.visible(outside, left(19.0, 31.0)).any()
    # equals the caller's alternative: the closest hit's distance against the pair's
    rec = scene.trace_segments(a, left(19.0, 31.0) - a, 1.0)
    assert (rec["material"] == 3).all() and (rec["t"] > 0).all() and (rec["t"] < 1).all() and (rec["voxel"][:, 0] == 16).all()
    # torch tensors in, a torch tensor out
    ta, tb = torch.from_numpy(a).to(engine.torch_device), torch.from_numpy(b).to(engine.torch_device)
    v = scene.visible(ta, tb)
    assert isinstance(v, torch.Tensor) and v.dtype == torch.bool and bool(v.all())
    with pytest.raises(ValueError, match="both"):                           # one of each is refused by name, not by numpy
        scene.visible(ta, b)
    scene.destroy()
