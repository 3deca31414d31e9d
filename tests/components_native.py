"""Host build of csrc/vrt_components.h (tests/native/components_host.cpp) for the component tests."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "components_host.cpp")
LIB = os.path.join(ROOT, "tests", "native", "libcomponents_host.so")
HDRS = [os.path.join(ROOT, "voxel-raytracing_amd", "csrc", n) for n in ("vrt_components.h", "vrt_brush.h")]

_lib = None


def components_host():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB) or any(os.path.getmtime(LIB) < os.path.getmtime(p) for p in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-fPIC", "-shared", "-o", LIB, SRC])
    l = C.CDLL(LIB)
    V = C.c_void_p
    l.comp_args_ok_c.argtypes = [C.c_int32, C.c_int32, C.c_uint32, V]
    l.comp_filter_ok_c.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32]
    l.comp_sides_ok_c.argtypes = [V]
    l.comp_key_c.argtypes = [C.c_int32, C.c_uint32]
    l.comp_key_c.restype = C.c_uint32
    l.comp_record_bytes_c.restype = C.c_uint32
    l.comp_record_offsets_c.argtypes = [V]
    l.comp_record_offsets_c.restype = None
    l.comp_forward_c.argtypes = [C.c_int32, V, V]
    l.comp_forward_c.restype = None
    l.comp_run_c.argtypes = [V, V, C.c_int32, C.c_int32, C.c_uint32, V, V, V, C.c_uint64, V, V]
    l.comp_filter_c.argtypes = [V, V, C.c_int32, C.c_int32, C.c_uint32, V, V, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, V]
    _lib = l
    return l


def _arr(v, dtype):
    return np.asarray([int(t) for t in v], dtype)


def args_ok(match, conn, flags, size):
    s = _arr(size, np.uint32)
    return bool(components_host().comp_args_ok_c(match, conn, flags, s.ctypes.data))


def filter_ok(mn, mx, fa, fn, flags):
    return bool(components_host().comp_filter_ok_c(mn, mx, fa, fn, flags))


def sides_ok(cs):
    s = _arr(cs, np.uint32)
    return bool(components_host().comp_sides_ok_c(s.ctypes.data))


def key(match, vid):
    return int(components_host().comp_key_c(match, vid))


def record_layout():
    """-> (sizeof, {field: offset}) of the header's CompRecord"""
    off = np.zeros(7, np.uint32)
    components_host().comp_record_offsets_c(off.ctypes.data)
    return int(components_host().comp_record_bytes_c()), dict(zip(("root", "id", "voxels", "lo", "size", "faces", "reserved"), (int(v) for v in off)))


def forward(conn):
    out, n = np.zeros(39, np.int32), np.zeros(1, np.uint32)
    components_host().comp_forward_c(conn, out.ctypes.data, n.ctypes.data)
    return [tuple(int(v) for v in out[3 * k:3 * k + 3]) for k in range(int(n[0]))]


def components(vol, match, conn, bounds, dtype, flags=0):
    """The header's twin -> (rc, records as a structured array of `dtype`, result, labels [z, y, x] over the clipped bounds or None)"""
    v = np.ascontiguousarray(vol, np.uint8)
    D, H, W = v.shape
    lo, size = ((0, 0, 0), (W, H, D)) if bounds is None else bounds
    dim, l, s = _arr((W, H, D), np.int32), _arr(lo, np.int32), _arr(size, np.uint32)
    res = np.zeros(9, np.int64)
    rec = np.zeros(v.size, dtype)
    labels = np.zeros(v.size, np.uint32)
    rc = components_host().comp_run_c(dim.ctypes.data, v.ctypes.data, match, conn, flags, l.ctypes.data, s.ctypes.data, rec.ctypes.data, rec.size,
                                      labels.ctypes.data, res.ctypes.data)
    r = [int(t) for t in res]
    nv = r[6] * r[7] * r[8]
    return rc, rec[:r[0]].copy(), {"components": r[0], "voxels": r[1], "largest": r[2]}, labels[:nv].reshape(r[8], r[7], r[6]).copy() if nv else None


def filter_components(vol, vid, match, conn, bounds=None, min_voxels=0, max_voxels=2 ** 64 - 1, faces_all=0, faces_none=0, keep_largest=False, measure=False):
    """-> (rc, the volume after, the result as VoxelScene.filter_components returns it)"""
    out = np.ascontiguousarray(vol, np.uint8).copy()
    D, H, W = out.shape
    lo, size = ((0, 0, 0), (W, H, D)) if bounds is None else bounds
    dim, l, s = _arr((W, H, D), np.int32), _arr(lo, np.int32), _arr(size, np.uint32)
    res = np.zeros(9, np.int64)
    rc = components_host().comp_filter_c(dim.ctypes.data, out.ctypes.data, match, conn, 0, l.ctypes.data, s.ctypes.data, min_voxels, max_voxels, faces_all,
                                         faces_none, (1 if keep_largest else 0) | (2 if measure else 0), vid, res.ctypes.data)
    r = [int(t) for t in res]
    return rc, out, {"components": r[0], "voxels": r[1], "changed": r[2], "lo": tuple(r[3:6]), "size": tuple(r[6:9])}
