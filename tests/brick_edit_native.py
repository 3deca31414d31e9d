"""Host build of csrc/vrt_brick_edit.h (tests/native/brick_edit_host.cpp) for the brick-scene edit tests."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "brick_edit_host.cpp")
LIB = os.path.join(ROOT, "tests", "native", "libbrick_edit_host.so")
HDRS = [os.path.join(ROOT, "voxel-raytracing_amd", "csrc", n) for n in ("vrt_brick_edit.h", "vrt_edit.h")]


def brick_edit_host():
    if not os.path.exists(LIB) or any(os.path.getmtime(LIB) < os.path.getmtime(p) for p in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", LIB, SRC])
    l = C.CDLL(LIB)
    l.brick_edit_sweep.argtypes = [C.c_uint32, C.c_int, C.c_void_p]
    l.brick_edit_sweep.restype = None
    l.brick_edit_in_place_c.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    l.brick_edit_spans.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    l.brick_edit_spans.restype = None
    return l


def _box(lo, size):
    lo = np.asarray(lo, np.int32)
    return lo, (lo + np.asarray(size, np.int32)).astype(np.int32)


def in_place(l, nb, lo, size):
    """the rule of vrt_brick_edit.h for an edit that changed some brick's occupancy; nb: bricks (x, y, z); lo, size: voxels"""
    lo, hi = _box(lo, size)
    return bool(l.brick_edit_in_place_c(int(nb[0]), int(nb[1]), int(nb[2]), lo.ctypes.data, hi.ctypes.data))


def spans(l, nb, lo, size):
    """{'T': [(lo, hi)] * 3, 'F': ..., 'R': [octant][axis], 'E': ..., 'Q': ...} in bricks"""
    lo, hi = _box(lo, size)
    out = np.zeros((78, 2), np.int32)
    l.brick_edit_spans(int(nb[0]), int(nb[1]), int(nb[2]), lo.ctypes.data, hi.ctypes.data, out.ctypes.data)
    s = [tuple(int(v) for v in r) for r in out]
    return {"T": s[0:3], "F": s[3:6], "R": [s[6 + 9 * o:9 + 9 * o] for o in range(8)], "E": [s[9 + 9 * o:12 + 9 * o] for o in range(8)],
            "Q": [s[12 + 9 * o:15 + 9 * o] for o in range(8)]}
