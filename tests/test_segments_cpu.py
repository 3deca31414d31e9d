"""Ray segments without a GPU: the per-ray code of the segment kernels (csrc/vrt_query_seg.h) compiled for the host against
tests/segment_reference.py -- itself held to the oracle's vo_trace_ray first --, the iteration bound that sets a wave's budget, and
the C-ABI surface of vrt_trace_segments / vrt_occluded_segments."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import segment_common as SC
import segment_reference as SR
from ray_query_common import EDGE_CLASSES, edge_rays, open_set

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
SRC = os.path.join(NATIVE, "segment_host.cpp")
LIB = os.path.join(NATIVE, "libsegment_host.so")
DEPS = [SRC, os.path.join(NATIVE, "traverse_host.cpp"), os.path.join(ROOT, "include", "vrt.h")] + \
       [os.path.join(ROOT, "voxel-raytracing_amd", "csrc", h) for h in
        ("vrt_query_seg.h", "vrt_query.h", "vrt_traverse.h", "vrt_march_df.h", "vrt_march_fast.h", "vrt_march_brick.h", "vrt_march_literal.h",
         "vrt_volume.h", "vrt_dda.h", "vrt_spec.h")]


@pytest.fixture(scope="module")
def sh():
    if not os.path.exists(LIB) or any(os.path.getmtime(LIB) < os.path.getmtime(p) for p in DEPS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", LIB, SRC])
    l = C.CDLL(LIB)
    l.th_create.restype = C.c_void_p; l.th_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    l.thb_create.restype = C.c_void_p; l.thb_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    l.th_destroy.argtypes = [C.c_void_p]; l.thb_destroy.argtypes = [C.c_void_p]
    l.sh_segments.restype = None
    l.sh_segments.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_void_p] * 5
    l.sh_bound.restype = None
    l.sh_bound.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    l.sh_sizeof_ray_hits.restype = C.c_size_t
    return l


def host_segments(sh, h, bricks, starts, dirs, t_max, max_steps, anyhit=False, own_budget=False):
    n = len(starts)
    out = {"material": np.zeros(n, np.uint8), "pos": np.zeros((n, 3), np.float32), "voxel": np.zeros((n, 3), np.int32),
           "normal": np.zeros((n, 3), np.int8), "t": np.zeros(n, np.float32)}
    sh.sh_segments(h, int(bricks), int(anyhit), int(own_budget), n, starts.ctypes.data, dirs.ctypes.data, t_max.ctypes.data, max_steps,
                   out["material"].ctypes.data, out["pos"].ctypes.data, out["voxel"].ctypes.data, out["normal"].ctypes.data, out["t"].ctypes.data)
    return out


def host_bound(sh, h, bricks, starts, dirs, t_max):
    out = np.zeros(len(starts), np.float32)
    sh.sh_bound(h, int(bricks), len(starts), starts.ctypes.data, dirs.ctypes.data, t_max.ctypes.data, out.ctypes.data)
    return out


@pytest.fixture(scope="module", params=SC.VOLUMES, ids=lambda v: "x".join(str(d) for d in v[1]))
def case(request, oracle):
    return SC.segment_case(oracle, *request.param)


def test_segment_records_match_reference(sh, case):
    """Every plane and t of query_segment_ray -- VRT_TRAVERSAL_DF on the dense volume, the brick march on the same content in bricks --
    equal the reference under the limits, bit for bit, for 5000 rays and max_steps in (512, 37, 1); the any-hit form equals
    material != 0.  The batch holds, at 512: >= 5 % kept hits, >= 5 % hits the limit drops, >= 5 % rays that miss anyway, and >= 100
    hits each whose limit is t_hit exactly and the float below it."""
    W, H, D = case["dims"]
    vol, starts, dirs, t_max, cls = (case[k] for k in ("vol", "starts", "dirs", "t_max", "cls"))
    assert len(starts) == 5000
    hit512 = case["ref"][512]["material"] != 0
    kept = case["exp"][512]["material"] != 0
    share = (float(kept.mean()), float((hit512 & ~kept).mean()), float((~hit512).mean()))
    print(f"\n{case['dims']}: ray seed {case['ray_seed']}, kept / dropped by t_max / miss anyway = {share[0]:.3f} / {share[1]:.3f} / {share[2]:.3f}; "
          f"exact {int((hit512 & (cls == 0)).sum())}, below {int((hit512 & (cls == 1)).sum())}")
    assert min(share) >= 0.05, share
    assert (hit512 & (cls == 0)).sum() >= 100 and (hit512 & (cls == 1)).sum() >= 100
    assert kept[hit512 & (cls == 0)].all() and not kept[hit512 & (cls == 1)].any()        # the compare is <=, on the bit
    assert np.isnan(t_max).any() and np.isinf(t_max).any() and (t_max == 0).any() and (t_max == -1).any()
    assert (kept & (t_max == 0)).any() or not ((case["ref"][512]["t"] == 0) & hit512 & (cls == 5)).any()
    hd, hb = sh.th_create(vol.ctypes.data, W, H, D), sh.thb_create(vol.ctypes.data, W, H, D)
    for ms in SC.BUDGETS:
        exp = case["exp"][ms]
        for bricks, h in ((0, hd), (1, hb)):
            got = host_segments(sh, h, bricks, starts, dirs, t_max, ms)
            bad = SC.planes_differ(got, exp)
            assert bad.size == 0, (bricks, ms, bad[:5], {k: v[bad[:3]] for k, v in got.items()}, {k: exp[k][bad[:3]] for k in got},
                                   starts[bad[:3]], dirs[bad[:3]], t_max[bad[:3]])
            occ = host_segments(sh, h, bricks, starts, dirs, t_max, ms, anyhit=True)["material"]
            assert (occ == exp["occluded"]).all() and (occ == (exp["material"] != 0)).all(), (bricks, ms)
            # every ray marched with its own segment's budget, the tightest a wave can get: nothing changes
            assert SC.planes_differ(host_segments(sh, h, bricks, starts, dirs, t_max, ms, own_budget=True), exp).size == 0, (bricks, ms)
            assert (host_segments(sh, h, bricks, starts, dirs, t_max, ms, anyhit=True, own_budget=True)["material"] == occ).all(), (bricks, ms)
            # +inf keeps every hit: the record is the reference's own
            inf = np.full(len(starts), np.inf, np.float32)
            assert SC.planes_differ(host_segments(sh, h, bricks, starts, dirs, inf, ms), SR.segment_records(case["ref"][ms], inf)).size == 0
    sh.th_destroy(hd); sh.thb_destroy(hb)


def _assert_bound(sh, h, bricks, ref, starts, dirs, t_max, what):
    with np.errstate(invalid="ignore"):
        kept = (ref["material"] != 0) & (ref["t"] <= t_max)
    bound = host_bound(sh, h, bricks, starts, dirs, t_max)
    assert not np.isnan(bound).any() and (bound >= 8.0).all()
    bad = np.flatnonzero(kept & ~(ref["steps"].astype(np.float64) <= bound.astype(np.float64)))
    assert bad.size == 0, (what, bad[:5], ref["steps"][bad[:5]], bound[bad[:5]], starts[bad[:3]], dirs[bad[:3]], t_max[bad[:3]])
    return kept, bound


def test_segment_bound_covers_every_kept_hit(sh, case):
    """query_segment_bound: a kept hit in iteration k needs a budget of k + 1, the voxels the oracle fetched for it; the bound is at
    least that for every kept hit of the batch, under its drawn limits and under t_max = t_hit, the tightest limit that keeps.  Short
    segments get budgets well below their rays': the bound at t_hit is printed beside the bound at +inf."""
    W, H, D = case["dims"]
    vol, starts, dirs, t_max = (case[k] for k in ("vol", "starts", "dirs", "t_max"))
    ref = case["ref"][512]
    hd, hb = sh.th_create(vol.ctypes.data, W, H, D), sh.thb_create(vol.ctypes.data, W, H, D)
    for bricks, h in ((0, hd), (1, hb)):
        _assert_bound(sh, h, bricks, ref, starts, dirs, t_max, "drawn")
        kept, tight = _assert_bound(sh, h, bricks, ref, starts, dirs, ref["t"].copy(), "exact")
        full = host_bound(sh, h, bricks, starts, dirs, np.full(len(starts), np.inf, np.float32))
        assert (tight[kept] <= full[kept]).all()
        print(f"\n{case['dims']} bricks={bricks}: median bound at t_hit {np.median(tight[kept]):.1f}, at +inf {np.median(full[kept]):.1f}, "
              f"median iterations {np.median(ref['steps'][kept]):.0f}")
        # a NaN limit is not bounded (and keeps nothing)
        assert np.isinf(host_bound(sh, h, bricks, starts[:8], dirs[:8], np.full(8, np.nan, np.float32))).all()
    sh.th_destroy(hd); sh.thb_destroy(hb)


@pytest.mark.parametrize("cls", EDGE_CLASSES)
def test_segment_bound_on_edge_classes(sh, oracle, cls):
    """The same for the ray classes a pinhole cannot produce (ray_query_common.edge_rays, the open set removed), 2000 rays each on the
    40 x 32 x 56 volume at max_steps 1024 and t_max = t_hit: the reference equals the oracle on them, the records equal the
    reference, and no kept hit lies outside its bound -- a far origin's bound is +inf."""
    seed, dims, fill = SC.VOLUMES[0]
    W, H, D = dims
    vol = SC.make_volume(seed, dims, fill)
    osn = oracle.OracleScene(vol, np.zeros((256, 5), np.float32))
    starts, dirs = edge_rays(np.random.default_rng(4000 + EDGE_CLASSES.index(cls)), 2000, dims, cls, vol)
    comp, rays = open_set(starts, dirs, dims)
    assert not comp.any() and not rays.any()
    ref = SR.trace(vol, starts, dirs, 1024)
    bad = SR.differs_from_oracle(ref, SR.oracle_trace(oracle, osn, starts, dirs, 1024))
    assert bad.size == 0, (cls, bad[:5], starts[bad[:3]], dirs[bad[:3]])
    hit = ref["material"] != 0
    assert hit.any(), cls
    t_max = ref["t"].copy()
    exp = SR.segment_records(ref, t_max)
    assert (exp["material"] != 0)[hit].all()
    hd, hb = sh.th_create(vol.ctypes.data, W, H, D), sh.thb_create(vol.ctypes.data, W, H, D)
    for bricks, h in ((0, hd), (1, hb)):
        for own in (False, True):
            got = host_segments(sh, h, bricks, starts, dirs, t_max, 1024, own_budget=own)
            bad = SC.planes_differ(got, exp)
            assert bad.size == 0, (cls, bricks, own, bad[:5], {k: v[bad[:3]] for k, v in got.items()}, {k: exp[k][bad[:3]] for k in got})
        _, bound = _assert_bound(sh, h, bricks, ref, starts, dirs, t_max, cls)
        if cls == "far":
            assert np.isinf(bound[(np.abs(starts) > 2.0 ** 20).any(axis=1)]).all()
    sh.th_destroy(hd); sh.thb_destroy(hb)


def test_c_abi_surface(sh, vrt):
    """The two symbols are exported and listed in _capi.SYMBOLS; vrt_ray_hits keeps its 32 bytes; argument errors come back as
    VRT_ERR_INVALID with query_args' messages in its order, plus "NULL t_max", before anything touches a context or a device (there
    is none here); the Python mirrors exist."""
    lib = vrt.lib()
    for name in ("vrt_trace_segments", "vrt_occluded_segments"):
        assert name in vrt._capi.SYMBOLS and hasattr(C.CDLL(vrt._capi.LIB_PATH), name)
    RH = vrt._capi.RayHits
    assert C.sizeof(RH) == sh.sh_sizeof_ray_hits() == 32
    INVALID = 1
    buf = (C.c_uint8 * 64)()                       # stands for any non-NULL pointer: the calls below return before they look at it
    p = C.cast(buf, C.c_void_p)
    planes = RH(material=p)
    err = lambda: lib.vrt_last_error().decode()
    trace, occ = lib.vrt_trace_segments, lib.vrt_occluded_segments
    # scalars first, whatever else is passed
    assert trace(None, None, -1, None, None, None, 512, None, None) == INVALID and "n < 0" in err()
    assert occ(None, None, -1, None, None, None, 512, None) == INVALID and "n < 0" in err()
    assert trace(p, p, vrt._capi.MAX_QUERY_RAYS + 1, p, p, p, 512, C.byref(planes), p) == INVALID and "2^28" in err()
    assert occ(p, p, vrt._capi.MAX_QUERY_RAYS + 1, p, p, p, 512, p) == INVALID and "2^28" in err()
    assert trace(p, p, 4, p, p, p, 0, C.byref(planes), p) == INVALID and "max_steps" in err()
    assert occ(p, p, 4, p, p, p, 0, p) == INVALID and "max_steps" in err()
    # NULL arguments, then NULL t_max, then no output
    assert trace(None, p, 4, p, p, p, 512, C.byref(planes), p) == INVALID and "NULL argument" in err()
    assert trace(p, p, 4, p, None, None, 512, C.byref(planes), p) == INVALID and "NULL argument" in err()
    assert occ(p, None, 4, p, p, None, 512, None) == INVALID and "NULL argument" in err()
    assert trace(p, p, 4, p, p, None, 512, None, None) == INVALID and "NULL t_max" in err() and "vrt_trace_segments" in err()
    assert occ(p, p, 4, p, p, None, 512, None) == INVALID and "NULL t_max" in err() and "vrt_occluded_segments" in err()
    assert trace(p, p, 4, p, p, p, 512, None, None) == INVALID and "no output plane" in err()
    assert trace(p, p, 4, p, p, p, 512, C.byref(RH()), None) == INVALID and "no output plane" in err()
    assert occ(p, p, 4, p, p, p, 512, None) == INVALID and "no output plane" in err()
    # the Python mirrors exist
    for m in ("trace_segments", "occluded", "visible"):
        assert callable(getattr(vrt.VoxelScene, m))
    import inspect
    assert "t_max" in inspect.signature(vrt.VoxelScene.occluded).parameters
