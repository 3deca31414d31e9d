"""The product's traversal header (csrc/vrt_traverse.h) compiled for the host: DENSE, BITMASK and the exact
JUMP strategy against the oracle's literal DDA on large ray sets -- hit cell, mask, material, the sideDist
bit patterns at the hit, and (DENSE/BITMASK) the fetch count must be identical."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "traverse_host.cpp")
LIB = os.path.join(ROOT, "tests", "native", "libtraverse_host.so")
HDRS = [os.path.join(ROOT, "voxel-raytracing_amd", "csrc", h) for h in
        ("vrt_traverse.h", "vrt_march_df.h", "vrt_march_fast.h", "vrt_march_brick.h", "vrt_march_literal.h",
         "vrt_volume.h", "vrt_dda.h", "vrt_spec.h")]


@pytest.fixture(scope="module")
def th():
    lib = LIB
    if os.environ.get("VRT_TH_SANITIZE") == "1":
        # AddressSanitizer + UBSan build of the same code (CPU only; run with LD_PRELOAD=$(gcc -print-file-name=libasan.so)
        # ASAN_OPTIONS=detect_leaks=0): out-of-bounds reads of the padded clearance fields, the occupancy pyramid, ...
        lib = LIB.replace(".so", "_san.so")
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-fPIC", "-shared", "-o", lib, SRC])
    elif not os.path.exists(LIB) or any(os.path.getmtime(LIB) < os.path.getmtime(p) for p in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", LIB, SRC])
    l = C.CDLL(lib)
    l.th_create.restype = C.c_void_p
    l.th_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    l.th_destroy.argtypes = [C.c_void_p]
    l.th_trace.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    l.thb_create.restype = C.c_void_p
    l.thb_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    l.thb_destroy.argtypes = [C.c_void_p]
    l.thb_trace.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p]
    return l


def trace(th, h, trav, starts, dirs, max_steps=512):
    starts = np.ascontiguousarray(starts, np.float32); dirs = np.ascontiguousarray(dirs, np.float32)
    n = len(starts)
    out = np.zeros((n, 12), np.uint32); stats = np.zeros(6, np.uint64)
    th.th_trace(h, trav, n, starts.ctypes.data, dirs.ctypes.data, max_steps, out.ctypes.data, stats.ctypes.data)
    return out, stats


def oracle_trace(oracle, osn, starts, dirs, max_steps=512):
    out = np.zeros((len(starts), 12), np.uint32)
    for i, (s, d) in enumerate(zip(starts, dirs)):
        h = oracle.trace_ray(osn, s, d, max_steps)
        hit = h.material != 0
        side = np.array(list(h.side), np.float32).view(np.uint32)
        p0 = np.array(list(h.p0), np.float32).view(np.uint32)
        out[i] = [h.material, h.mask if hit else 0] + ([np.uint32(v & 0xFFFFFFFF) for v in h.voxel] if hit else [0, 0, 0]) + \
                 (list(side) if hit else [0, 0, 0]) + list(p0) + [h.steps]
    return out


def _rays(rng, n, dims, inside_frac=0.3):
    W, H, D = dims
    starts = np.empty((n, 3), np.float32); dirs = np.empty((n, 3), np.float32)
    for i in range(n):
        if rng.random() < inside_frac:
            s = rng.uniform([0, 0, 0], [W, H, D])
        else:
            s = rng.uniform([-W, -H, -D], [2 * W, 2 * H, 2 * D])
        t = rng.uniform([0, 0, 0], [W, H, D])
        d = t - s
        d /= np.linalg.norm(d) + 1e-9
        if rng.random() < 0.15:
            d *= rng.uniform(0.3, 2.0)                     # AO-style un-normalised directions
        if rng.random() < 0.08:
            d[rng.integers(0, 3)] = 0.0                    # axis-parallel component
        if rng.random() < 0.05:
            s = np.round(s); d = np.sign(d) * np.array([1.0, 1.0, 1.0]) * rng.choice([0.5, 1.0])   # lattice ties
        starts[i], dirs[i] = s, d
    return starts, dirs


@pytest.mark.parametrize("seed,dims,fill", [(1, (40, 33, 52), 0.002), (2, (64, 64, 64), 0.02), (3, (130, 20, 70), 0.0005), (4, (17, 9, 5), 0.1)])
def test_strategies_match_oracle_random_rays(th, oracle, seed, dims, fill):
    rng = np.random.default_rng(seed)
    W, H, D = dims
    vol = ((rng.random((D, H, W)) < fill) * rng.integers(1, 256, (D, H, W))).astype(np.uint8)
    vol[D // 2:, : max(1, H // 8), :] |= np.uint8(7)        # a slab so that long empty runs end in hits
    h = th.th_create(vol.ctypes.data, W, H, D)
    osn = oracle.OracleScene(vol, np.zeros((256, 5), np.float32))
    starts, dirs = _rays(rng, 6000, dims)
    for max_steps in (512, 64, 37):
        exp = oracle_trace(oracle, osn, starts, dirs, max_steps)
        for trav, name in ((1, "DENSE"), (2, "BITMASK"), (4, "DF"), (3, "JUMP"), (5, "DFJ")):
            got, stats = trace(th, h, trav, starts, dirs, max_steps)
            cols = slice(0, 12) if trav not in (3, 5) else slice(0, 11)  # JUMP / DFJ fetch counts are upper bounds
            bad = np.flatnonzero((got[:, cols] != exp[:, cols]).any(axis=1))
            assert bad.size == 0, (name, max_steps, bad[:5], got[bad[:3]], exp[bad[:3]], starts[bad[:3]], dirs[bad[:3]])
            if trav in (3, 5):
                assert (got[:, 11] >= exp[:, 11]).all()
    th.th_destroy(h)


def test_jump_statistics_treehouse(th, oracle, vrt):
    """Primary rays of the bench frame (subsampled): exact agreement + the iteration savings JUMP is for."""
    from helpers import camera_push
    vol = vrt.synthetic.treehouse(256, seed=2)
    h = th.th_create(vol.ctypes.data, 256, 256, 256)
    osn = oracle.OracleScene(vol, np.zeros((256, 5), np.float32))
    pos, yaw, pitch = vrt.synthetic.default_camera_for(256, 256, 256)
    push = camera_push(vrt, (256, 256, 256), (1920, 1080), pos=pos, yaw=yaw, pitch=pitch)
    pix = [(x, y) for y in range(4, 1080, 24) for x in range(5, 1920, 24)]
    rays = [oracle.primary_ray(push, x, y) for x, y in pix]
    starts = np.array([r[0] for r in rays]); dirs = np.array([r[1] for r in rays])
    exp = oracle_trace(oracle, osn, starts, dirs)
    got, stats = trace(th, h, 3, starts, dirs)
    assert (got[:, :11] == exp[:, :11]).all()
    literal_iters = int(exp[:, 11].sum())
    jump_iters = int(stats[:4].sum())
    print(f"\nliteral DDA iterations {literal_iters}, JUMP iterations {jump_iters} "
          f"(literal {stats[0]}, 4^3 {stats[1]}, 16^3 {stats[2]}, 64^3 {stats[3]}), retraces {stats[4]}, lookups {stats[5]}")
    assert jump_iters * 2 < literal_iters
    th.th_destroy(h)


@pytest.mark.parametrize("seed,dims,fill", [(11, (40, 32, 56), 0.002), (12, (64, 64, 64), 0.02), (13, (128, 24, 72), 0.0005), (14, (16, 8, 8), 0.1)])
def test_brick_march_matches_oracle_random_rays(th, oracle, seed, dims, fill):
    """trace_brick (the march over the two-level clearance of a brick scene) on the host against the oracle's literal DDA of the
    dense volume: hit cell, mask, material, sideDist bits and fetch count identical; the any-hit form agrees on material and
    fetches and never needs more look-ups."""
    rng = np.random.default_rng(seed)
    W, H, D = dims
    vol = ((rng.random((D, H, W)) < fill) * rng.integers(1, 256, (D, H, W))).astype(np.uint8)
    vol[D // 2:, : max(1, H // 8), :] |= np.uint8(7)
    vol[:8, :8, :8] = 0                                           # an empty corner brick next to the walls
    h = th.thb_create(vol.ctypes.data, W, H, D)
    osn = oracle.OracleScene(vol, np.zeros((256, 5), np.float32))
    starts, dirs = _rays(rng, 5000, dims)
    for max_steps in (512, 64, 37, 1):
        exp = oracle_trace(oracle, osn, starts, dirs, max_steps)
        out = np.zeros((len(starts), 12), np.uint32); lk = C.c_uint64()
        th.thb_trace(h, len(starts), np.ascontiguousarray(starts, np.float32).ctypes.data, np.ascontiguousarray(dirs, np.float32).ctypes.data,
                     max_steps, 0, out.ctypes.data, C.byref(lk))
        bad = np.flatnonzero((out != exp).any(axis=1))
        assert bad.size == 0, (max_steps, bad[:5], out[bad[:3]], exp[bad[:3]], starts[bad[:3]], dirs[bad[:3]])
        any_out = np.zeros_like(out); lk2 = C.c_uint64()
        th.thb_trace(h, len(starts), np.ascontiguousarray(starts, np.float32).ctypes.data, np.ascontiguousarray(dirs, np.float32).ctypes.data,
                     max_steps, 1, any_out.ctypes.data, C.byref(lk2))
        assert (any_out[:, 0] == exp[:, 0]).all() and (any_out[:, 11] == exp[:, 11]).all(), max_steps
        assert lk2.value <= lk.value
    th.thb_destroy(h)


def test_df_fast_layout_predicate_covers_every_offset(th):
    """The hand-written look-up loop forms 32-bit offsets from (W+2)(H+2) bytes in front of field 0; the host may only choose
    it while the largest of them (the 0xFF byte, a hit's id read, a prefetch one slice on) stays below 2^32.  Sizes either
    side of the boundary, the advisor's two (1498x1498x210, 480x480x2052) included: the old test 9*ndf + 256 <= 2^32 - 1
    accepted both although the sentinel offset wraps."""
    th.th_df_fast_layout_ok.argtypes = [C.c_int, C.c_int, C.c_int]
    th.th_df_fast_reach.restype = C.c_uint64
    th.th_df_fast_reach.argtypes = [C.c_int, C.c_int, C.c_int]
    for dims in [(1498, 1498, 210), (480, 480, 2052), (256, 256, 256), (512, 512, 512), (768, 768, 768), (780, 780, 780),
                 (781, 781, 781), (4096, 8, 8), (8, 4096, 8), (8, 8, 4096), (2894, 2894, 54), (1, 1, 1)]:
        ok, reach = th.th_df_fast_layout_ok(*dims), th.th_df_fast_reach(*dims)
        if ok:
            assert reach <= 0xFFFFFFFF, (dims, reach)
            assert (dims[0] + 2) * (dims[1] + 2) < (1 << 23)
    assert not th.th_df_fast_layout_ok(1498, 1498, 210) and th.th_df_fast_reach(1498, 1498, 210) > 0xFFFFFFFF
    assert not th.th_df_fast_layout_ok(480, 480, 2052) and th.th_df_fast_reach(480, 480, 2052) > 0xFFFFFFFF
    assert th.th_df_fast_layout_ok(256, 256, 256) and th.th_df_fast_layout_ok(512, 512, 512)
    # a sweep across the boundary along one axis: the predicate never accepts a volume whose reach wraps
    for d in range(1900, 2100, 3):
        if th.th_df_fast_layout_ok(480, 480, d):
            assert th.th_df_fast_reach(480, 480, d) <= 0xFFFFFFFF, d
