"""The volumes, ray batches and cameras of tests/extents_common.py without a GPU: the host builds of the marches (tests/native/
traverse_host.cpp through test_traverse_host.py) and of the ray queries (query_host.cpp through test_ray_query_cpu.py) run the
needle batches against the oracle, and the composition every batch and every camera must have is decided here, on the oracle's
results alone, before anything goes to a GPU (tests/test_gpu_extents.py asserts the same conditions again).

On the host mul24 is a plain multiply and the look-up loops' v_mad_i32_i24 do not exist: the 24-bit forms of the index
arithmetic are what only the GPU tier sees.  What this tier pins is everything else at 4096: the clearance fields and the
pyramid of the host builder, the DDA's float arithmetic at coordinates up to 4096, the brick march over 512 bricks."""
import numpy as np
import pytest

import extents_common as X
from helpers import metallic_palette
from ray_query_common import open_set, oracle_records, planes_differ
from test_ray_query_cpu import host_query, qh                      # noqa: F401  (fixtures that build and load the libraries)
from test_traverse_host import oracle_trace, th, trace             # noqa: F401


def needle_conditions(dims, sign, starts, records):
    """records: {budget: (planes, classes)} of oracle_records.  At 5000 at least 10 % of the rays hit a voxel within 64 of the far
    end from more than 3000 voxels away; at 1024 at least 10 % hit and at least 10 % exhaust the budget."""
    a = X.long_axis(dims)
    exp, cls = records[5000]
    along = exp["voxel"][:, a]
    far = (along >= dims[a] - 64) if sign > 0 else (along < 64)
    share = ((cls == 0) & far & (np.abs(along - starts[:, a]) > 3000)).mean()
    assert share >= 0.10, (dims, sign, share)
    _, cls = records[1024]
    assert (cls == 0).mean() >= 0.10 and (cls == 2).mean() >= 0.10, (dims, sign, (cls == 0).mean(), (cls == 2).mean())


def slab_conditions(dims, records):
    """in every batch at least 10 % of the hits lie at x >= 4000 or y >= 2000"""
    for ms, (exp, cls) in records.items():
        hit = cls == 0
        far = (exp["voxel"][:, 0] >= 4000) | (exp["voxel"][:, 1] >= 2000)
        assert hit.mean() >= 0.10 and (hit & far).sum() >= 0.10 * hit.sum(), (dims, ms, hit.mean(), (hit & far).sum(), hit.sum())


def frame_condition(hit_id, what):
    """at least 5 % of the pixels hit and at least 5 % miss"""
    share = float((hit_id != 0).mean())
    assert 0.05 <= share <= 0.95, (what, share)


def no_open_rays(starts, dirs, dims):
    comp, rays = open_set(starts, dirs, dims)
    assert not comp.any() and not rays.any()
    assert np.isfinite(starts).all() and np.isfinite(dirs).all()


ALL_NEEDLES = X.NEEDLES + X.RAGGED + [tuple(8 * n for n in nb) for nb in X.BRICK_NEEDLES]


@pytest.mark.parametrize("dims", ALL_NEEDLES, ids=lambda d: "x".join(str(v) for v in d))
def test_needle_rays_host_marches_match_oracle(th, qh, oracle, dims):     # noqa: F811
    """1000 rays per direction along a needle, at max_steps 1024, 1025 and 5000: DENSE, BITMASK, DF, JUMP and DFJ of the traversal
    header equal the oracle's literal DDA (cell, mask, material, sideDist bits; DENSE / BITMASK / DF the fetch count too), the
    query's per-ray function equals vo_trace_ray in every plane, on 4096 x 8 x 8 the brick march too, the any-hit form equals
    material != 0.  (mul24 is a plain multiply here: see the module's docstring.)"""
    W, H, D = dims
    vol = X.needle_volume(dims)
    a = X.long_axis(dims)
    assert vol.take(0, axis=2 - a).all() and vol.take(dims[a] - 1, axis=2 - a).all()          # the caps: cells 0 and 1023
    assert (vol == X.METAL).any() and (dims[a] - 1) >> 2 == 1023
    osn = oracle.OracleScene(vol, np.zeros((256, 5), np.float32))
    h = th.th_create(vol.ctypes.data, W, H, D)
    hq = qh.th_create(vol.ctypes.data, W, H, D)
    hb = qh.thb_create(vol.ctypes.data, W, H, D) if all(v % 8 == 0 for v in dims) else None
    for sign in (1, -1):
        starts, dirs = X.needle_rays(dims, sign)
        no_open_rays(starts, dirs, dims)
        along = starts[:, a] if sign > 0 else dims[a] - starts[:, a]
        assert (along < 0).any() and (np.abs(along - dims[a] / 2) < 50).any() and ((along > dims[a] - 100) & (along < dims[a])).any()
        records = {}
        for ms in X.BUDGETS:
            records[ms] = oracle_records(oracle, osn, starts, dirs, ms)
            exp12 = oracle_trace(oracle, osn, starts, dirs, ms)
            for trav, name in ((1, "DENSE"), (2, "BITMASK"), (4, "DF"), (3, "JUMP"), (5, "DFJ")):
                got, _ = trace(th, h, trav, starts, dirs, ms)
                cols = slice(0, 12) if trav not in (3, 5) else slice(0, 11)
                bad = np.flatnonzero((got[:, cols] != exp12[:, cols]).any(axis=1))
                assert bad.size == 0, (name, sign, ms, bad[:5], got[bad[:3]], exp12[bad[:3]], starts[bad[:3]], dirs[bad[:3]])
            exp = records[ms][0]
            for bricks, hh in ((0, hq), (1, hb)):
                if hh is None:
                    continue
                got = host_query(qh, hh, bricks, starts, dirs, ms)
                bad = planes_differ(got, exp)
                assert bad.size == 0, (bricks, sign, ms, bad[:5], {k: v[bad[:3]] for k, v in got.items()}, {k: v[bad[:3]] for k, v in exp.items()})
                occ = host_query(qh, hh, bricks, starts, dirs, ms, anyhit=True)["material"]
                assert (occ == (exp["material"] != 0)).all(), (bricks, sign, ms)
        needle_conditions(dims, sign, starts, records)
    th.th_destroy(h); qh.th_destroy(hq)
    if hb is not None:
        qh.thb_destroy(hb)


@pytest.mark.parametrize("dims,fast", X.SLABS, ids=lambda d: "x".join(str(v) for v in d) if isinstance(d, tuple) else str(d))
def test_slab_batches_hold_what_they_must(th, oracle, dims, fast):        # noqa: F811
    """the slab pair lies on either side of the host predicate, by one row; every ray of a batch crosses into another slice before it
    leaves the slab sideways, rays towards z = 0 and towards z = 2 both occur, all four corners hold origins, and the oracle's
    hits reach the far corner"""
    import ctypes as C
    th.th_df_fast_layout_ok.argtypes = [C.c_int, C.c_int, C.c_int]
    W, H, D = dims
    assert bool(th.th_df_fast_layout_ok(*dims)) == fast
    assert ((W + 2) * (H + 2) == (1 << 23) - 4096) if fast else ((W + 2) * (H + 2) == 1 << 23)
    vol = X.slab_volume(dims)
    assert vol[:, H - 1, W - 1].all() and vol[:, H - 3:, W - 3:].all()
    starts, dirs = X.slab_rays(dims)
    no_open_rays(starts, dirs, dims)
    size = np.array(dims, np.float64)
    with np.errstate(divide="ignore"):
        t_out = np.where(dirs > 0, (size - starts) / dirs, -starts / dirs)[:, :2].min(axis=1)          # leaves through a side in x or y
        t_z = np.where(dirs[:, 2] > 0, (2.0 - starts[:, 2]) / dirs[:, 2], (1.0 - starts[:, 2]) / dirs[:, 2])
    assert (t_z < t_out).all() and (dirs[:, 2] > 0).any() and (dirs[:, 2] < 0).any()
    for cx in (0, 1):
        for cy in (0, 1):
            near = (np.abs(starts[:, 0] - cx * W) < 41) & (np.abs(starts[:, 1] - cy * H) < 41)
            assert near.sum() >= len(starts) // 5
    osn = oracle.OracleScene(vol, np.zeros((256, 5), np.float32))
    slab_conditions(dims, {ms: oracle_records(oracle, osn, starts, dirs, ms) for ms in X.BUDGETS})


@pytest.mark.parametrize("dims", ALL_NEEDLES + [d for d, _ in X.SLABS], ids=lambda d: "x".join(str(v) for v in d))
def test_cameras_see_hits_and_sky(vrt, oracle, dims):
    """every camera, frame size and setting of the GPU tier's frames: by the oracle's hit_id at least 5 % of the pixels hit and at
    least 5 % miss"""
    slab = dims[2] == 3
    vol = X.slab_volume(dims) if slab else X.needle_volume(dims)
    osn = oracle.OracleScene(vol, metallic_palette(vrt))
    for cam in (X.slab_cameras(dims) if slab else X.needle_cameras(dims)):
        for res in X.FRAMES:
            push = X.push_of(vrt, dims, res, cam)
            for name, st in X.render_settings(vrt, res):
                if name.startswith("defaults"):
                    st = vrt.VoxelRenderSettings.primary_only(res)          # hit_id is the primary ray's: the budget decides it
                    st.traceSettings.maxRaySteps = 5000 if "5000" in name else 1024
                exp = oracle.render(osn, push, oracle.params_from(st.to_c()), planes=["hit_id"], nthreads=4)
                frame_condition(exp["hit_id"], (dims, cam[0], res, name))
