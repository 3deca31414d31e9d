"""Host build of csrc/vrt_morph.h (tests/native/morph_host.cpp) for the morphology tests."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "morph_host.cpp")
LIB = os.path.join(ROOT, "tests", "native", "libmorph_host.so")
HDRS = [os.path.join(ROOT, "voxel-raytracing_amd", "csrc", n) for n in ("vrt_morph.h", "vrt_brush.h")]

_lib = None


def morph_host():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB) or any(os.path.getmtime(LIB) < os.path.getmtime(p) for p in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-fPIC", "-shared", "-o", LIB, SRC])
    l = C.CDLL(LIB)
    V = C.c_void_p
    l.morph_run_c.argtypes = [V, V, C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.c_uint32, V, V, V]
    l.morph_args_ok_c.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.c_uint32, V]
    l.morph_sides_ok_c.argtypes = [V]
    l.morph_halo_c.argtypes = [C.c_int32, C.c_int32]
    l.morph_halo_c.restype = C.c_uint32
    l.morph_phases_c.argtypes = [C.c_int32]
    l.morph_phases_c.restype = C.c_uint32
    l.morph_phase_erodes_c.argtypes = [C.c_int32, C.c_uint32]
    l.morph_domain_c.argtypes = [V, V, C.c_uint32, V, V]
    l.morph_domain_c.restype = None
    l.morph_row_words_c.argtypes = [C.c_uint32]
    l.morph_row_words_c.restype = C.c_uint32
    l.morph_mask_words_c.argtypes = [V]
    l.morph_mask_words_c.restype = C.c_uint64
    l.morph_word_index_c.argtypes = [C.c_uint32] * 3 + [V]
    l.morph_word_index_c.restype = C.c_uint64
    l.morph_tiles_c.argtypes = [V, V]
    l.morph_tiles_c.restype = None
    l.morph_value_c.argtypes = [C.c_int32, C.c_int, C.c_uint32, C.c_uint32]
    l.morph_value_c.restype = C.c_uint32
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


def args_ok(op, conn, r, flags, vid, size):
    return bool(morph_host().morph_args_ok_c(op, conn, r, flags, vid, _u3(size)))


def sides_ok(cs):
    return bool(morph_host().morph_sides_ok_c(_u3(cs)))


def halo(op, r):
    return int(morph_host().morph_halo_c(op, r))


def phases(op):
    """-> one bool per phase: is it an erosion?"""
    l = morph_host()
    return [bool(l.morph_phase_erodes_c(op, p)) for p in range(int(l.morph_phases_c(op)))]


def domain(clo, cs, h):
    mlo, ms = np.zeros(3, np.int32), np.zeros(3, np.uint32)
    morph_host().morph_domain_c(_i3(clo), _u3(cs), h, mlo.ctypes.data, ms.ctypes.data)
    return [int(v) for v in mlo], [int(v) for v in ms]


def row_words(sx):
    return int(morph_host().morph_row_words_c(sx))


def mask_words(ms):
    return int(morph_host().morph_mask_words_c(_u3(ms)))


def word_index(w, ms):
    return int(morph_host().morph_word_index_c(int(w[0]), int(w[1]), int(w[2]), _u3(ms)))


def tiles(ms):
    nt = np.zeros(3, np.uint32)
    morph_host().morph_tiles_c(_u3(ms), nt.ctypes.data)
    return [int(v) for v in nt]


def value(op, bit, old, vid):
    return int(morph_host().morph_value_c(op, 1 if bit else 0, old, vid))


def morph(vol, op, r, conn=6, vid=0, bounds=None, border_solid=False, measure=False):
    """The header's tiled algorithm on the host -> (rc, the volume after, the result as VoxelScene.morph returns it)"""
    out = np.ascontiguousarray(vol, np.uint8).copy()
    D, H, W = out.shape
    lo, size = ((0, 0, 0), (W, H, D)) if bounds is None else bounds
    res = np.zeros(16, np.int64)
    rc = morph_host().morph_run_c(_i3((W, H, D)), out.ctypes.data, op, conn, r, (1 if border_solid else 0) | (2 if measure else 0), vid, _i3(lo), _u3(size),
                                  res.ctypes.data)
    v = [int(t) for t in res]
    return rc, out, {"added": v[0], "removed": v[1], "changed": v[2], "lo": tuple(v[3:6]), "size": tuple(v[6:9])}
