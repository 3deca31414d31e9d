"""Host build of csrc/vrt_edit.h (tests/native/edit_host.cpp) for the scene-edit tests."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "edit_host.cpp")
LIB = os.path.join(ROOT, "tests", "native", "libedit_host.so")
HDR = os.path.join(ROOT, "voxel-raytracing_amd", "csrc", "vrt_edit.h")


def edit_host():
    if not os.path.exists(LIB) or any(os.path.getmtime(LIB) < os.path.getmtime(p) for p in (SRC, HDR)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", LIB, SRC])
    l = C.CDLL(LIB)
    l.edit_sweep.argtypes = [C.c_uint32, C.c_int, C.c_void_p]
    l.edit_sweep.restype = None
    l.edit_in_place_c.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    return l


def in_place(l, dims, lo, size):
    lo = np.asarray(lo, np.int32)
    hi = (lo + np.asarray(size, np.int32)).astype(np.int32)
    return bool(l.edit_in_place_c(int(dims[0]), int(dims[1]), int(dims[2]), lo.ctypes.data, hi.ctypes.data))
