"""Host build of csrc/vrt_faces.h (tests/native/faces_host.cpp) for the surface-extraction tests, and the stand-alone program of its
generated volumes under the sanitizers (CPU only; it is a program of its own, nothing is preloaded)."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "faces_host.cpp")
LIB = os.path.join(ROOT, "tests", "native", "libfaces_host.so")
HDRS = [os.path.join(ROOT, "voxel-raytracing_amd", "csrc", n) for n in ("vrt_faces.h", "vrt_scene_read.h")]

MAIN_DIMS = [(70, 6, 5), (5, 131, 4), (9, 9, 9)]            # the volumes of faces_host.cpp's main()

_lib = None


def _stale(out):
    return not os.path.exists(out) or any(os.path.getmtime(out) < os.path.getmtime(p) for p in [SRC] + HDRS)


def faces_host():
    global _lib
    if _lib is not None:
        return _lib
    if _stale(LIB):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-fPIC", "-shared", "-o", LIB, SRC])
    l = C.CDLL(LIB)
    V = C.c_void_p
    l.faces_list_c.argtypes = [V, V, V, V, C.c_uint32, V, C.c_uint64, V]
    l.faces_list_c.restype = C.c_uint64
    l.faces_order_key_c.argtypes = [C.c_uint32] * 4 + [V]
    l.faces_order_key_c.restype = C.c_uint64
    l.faces_record_c.argtypes = [C.c_uint32] * 6
    l.faces_record_c.restype = C.c_uint64
    l.faces_record_valid_c.argtypes = [C.c_uint64]
    l.faces_quad_corner_c.argtypes = [C.c_uint64, C.c_uint32, V]
    l.faces_quad_corner_c.restype = None
    _lib = l
    return l


def faces(vol, lo, size, runs=True, closed=False):
    """-> (records uint64, counts uint64 (6,)) of a box of a dense volume [z][y][x]"""
    v = np.ascontiguousarray(vol, np.uint8)
    dim = np.asarray(v.shape[::-1], np.int32)
    l, s = np.asarray(lo, np.int32), np.asarray(size, np.uint32)
    flags = (1 if runs else 0) | (2 if closed else 0)
    counts = np.zeros(6, np.uint64)
    n = faces_host().faces_list_c(v.ctypes.data, dim.ctypes.data, l.ctypes.data, s.ctypes.data, flags, None, 0, counts.ctypes.data)
    rec = np.zeros(max(int(n), 1), np.uint64)
    assert faces_host().faces_list_c(v.ctypes.data, dim.ctypes.data, l.ctypes.data, s.ctypes.data, flags, rec.ctypes.data, n, counts.ctypes.data) == n
    return rec[:int(n)], counts


def quad(record):
    """the four corners of a record's quad, in voxels relative to the box's lo"""
    out = []
    for k in range(4):
        c = np.zeros(3, np.uint32)
        faces_host().faces_quad_corner_c(int(record), k, c.ctypes.data)
        out.append(tuple(int(t) for t in c))
    return out


def main_volume(v):
    """volume v of faces_host.cpp's main(), restated"""
    W, H, D = MAIN_DIMS[v]
    s, ids = 12345 + v, []
    for _ in range(W * H * D):
        s = (s * 1664525 + 1013904223) & 0xFFFFFFFF
        ids.append(0 if s >> 31 else 1 + (s >> 8) % 3)
    return np.array(ids, np.uint8).reshape(D, H, W)


def run_main_program(exe):
    """builds the sanitized stand-alone program as `exe` and runs it -> its lines as tuples (volume, box, flags, six counts, checksum)"""
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-DFACES_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, SRC])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-500:], p.stderr[-3000:])
    return [tuple(int(w) for w in line.split()) for line in p.stdout.splitlines()]
