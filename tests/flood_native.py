"""Host build of csrc/vrt_flood.h (tests/native/flood_host.cpp) for the flood tests."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "flood_host.cpp")
LIB = os.path.join(ROOT, "tests", "native", "libflood_host.so")
HDRS = [os.path.join(ROOT, "voxel-raytracing_amd", "csrc", n) for n in ("vrt_flood.h", "vrt_brush.h")]
ORDERS = {"forward": 0, "reverse": 1, "random": 2, "stale": 3}

_lib = None


def flood_host():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB) or any(os.path.getmtime(LIB) < os.path.getmtime(p) for p in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-fPIC", "-shared", "-o", LIB, SRC])
    l = C.CDLL(LIB)
    V = C.c_void_p
    l.flood_run_c.argtypes = [V, V, V, V, V, C.c_int32, C.c_int32, C.c_uint32, C.c_uint32, C.c_int, C.c_uint64, V]
    l.flood_args_ok_c.argtypes = [C.c_int32, C.c_int32, C.c_uint32, V]
    l.flood_sides_ok_c.argtypes = [V]
    l.flood_seed_inside_c.argtypes = [V, V, V]
    l.flood_passes_c.argtypes = [C.c_int32, C.c_uint32, C.c_uint32]
    l.flood_tiles_c.argtypes = [V, V]
    l.flood_tiles_c.restype = None
    l.flood_tile_index_c.argtypes = [C.c_uint32] * 3 + [V]
    l.flood_tile_index_c.restype = C.c_uint64
    l.flood_mask_byte_c.argtypes = [C.c_uint32] * 3 + [V]
    l.flood_mask_byte_c.restype = C.c_uint64
    l.flood_mask_bit_c.argtypes = [C.c_uint32]
    l.flood_mask_bit_c.restype = C.c_uint32
    l.flood_round_bound_c.argtypes = [V]
    l.flood_round_bound_c.restype = C.c_uint64
    l.flood_ext_row_c.argtypes = [C.c_int, V, V, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]
    l.flood_ext_row_c.restype = C.c_uint32
    l.flood_tile_relax_c.argtypes = [C.c_int, V, V]
    l.flood_wake_mask_c.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]
    l.flood_wake_mask_c.restype = C.c_uint32
    _lib = l
    return l


class _Arr:
    """a small array handed to C: ctypes takes its address through _as_parameter_ and the call keeps the object alive"""
    def __init__(self, v, dtype):
        self.a = np.asarray([int(t) for t in v], dtype)
        self._as_parameter_ = C.c_void_p(self.a.ctypes.data)


def _u3(v):
    return _Arr(v, np.uint32)


def _i3(v):
    return _Arr(v, np.int32)


def args_ok(match, conn, flags, size):
    return bool(flood_host().flood_args_ok_c(match, conn, flags, _u3(size)))


def sides_ok(cs):
    return bool(flood_host().flood_sides_ok_c(_u3(cs)))


def seed_inside(seed, clo, cs):
    return bool(flood_host().flood_seed_inside_c(_i3(seed), _i3(clo), _u3(cs)))


def passes(match, vid, seed_id):
    return bool(flood_host().flood_passes_c(match, vid, seed_id))


def tiles(cs):
    nt = np.zeros(3, np.uint32)
    flood_host().flood_tiles_c(_u3(cs), nt.ctypes.data)
    return [int(v) for v in nt]


def tile_index(t, nt):
    return int(flood_host().flood_tile_index_c(int(t[0]), int(t[1]), int(t[2]), _u3(nt)))


def mask_byte(r, nt):
    return int(flood_host().flood_mask_byte_c(int(r[0]), int(r[1]), int(r[2]), _u3(nt)))


def mask_bit(rx):
    return int(flood_host().flood_mask_bit_c(int(rx)))


def round_bound(cs):
    return int(flood_host().flood_round_bound_c(_u3(cs)))


def ext_row(conn, reached, nt, t, e):
    r = np.ascontiguousarray(reached, np.uint8)
    return int(flood_host().flood_ext_row_c(conn, r.ctypes.data, _u3(nt), int(t[0]), int(t[1]), int(t[2]), int(e)))


def tile_relax(conn, passable, ext):
    """-> (gained, the extended rows after the step)"""
    p, e = np.ascontiguousarray(passable, np.uint8), np.ascontiguousarray(ext, np.uint32).copy()
    g = flood_host().flood_tile_relax_c(conn, p.ctypes.data, e.ctypes.data)
    return bool(g), e


def wake_mask(conn, before, after, y, z):
    return int(flood_host().flood_wake_mask_c(conn, before, after, y, z))


def flood(vol, seed, vid, match=0, conn=6, bounds=None, measure=False, order="forward", rng=1):
    """The header's tiled algorithm on the host -> (rc, the volume after, the result as VoxelScene.flood returns it, rounds)"""
    out = np.ascontiguousarray(vol, np.uint8).copy()
    D, H, W = out.shape
    lo, size = ((0, 0, 0), (W, H, D)) if bounds is None else bounds
    res = np.zeros(16, np.int64)
    rc = flood_host().flood_run_c(_i3((W, H, D)), out.ctypes.data, _i3(seed), _i3(lo), _u3(size),
                                  match, conn, 1 if measure else 0, vid, ORDERS[order], rng, res.ctypes.data)
    r = [int(v) for v in res]
    return rc, out, {"region": r[0], "region_lo": tuple(r[1:4]), "region_size": tuple(r[4:7]), "seed_id": r[7], "changed": r[8],
                     "lo": tuple(r[9:12]), "size": tuple(r[12:15])}, r[15]
