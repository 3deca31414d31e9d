"""Shared by tests/test_upsample_cam_cpu.py, tests/test_raygen_offset_cpu.py and tests/test_gpu_upsample_cam.py: the host build of
the definitions (tests/native/upsample_cam_host.cpp), the scenes and the moving sequences temporal upsampling for ray cameras is
tested on, the oracle's frames over rays with sub-pixel offsets, and the definition (tests/upsample_cam_reference.py) run along a
sequence with ping-pong.

The scenes: floating_cubes(40, seed 1, count=50) with metallic ids for the perspective and the orthographic camera, and a closed
room -- a hollow 40^3 box with a few blocks standing in it -- around the panorama, so that every one of its rays hits."""
import ctypes as C
import os
import subprocess

import numpy as np

import reproject_common as rc
import upsample_cam_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
SRC = os.path.join(NATIVE, "upsample_cam_host.cpp")
LIB = os.path.join(NATIVE, "libupsample_cam_host.so")
DEPS = [SRC, os.path.join(ROOT, "include", "vrt.h")] + \
       [os.path.join(ROOT, "voxel-raytracing_amd", "csrc", h)
        for h in ("vrt_upsample_cam.h", "vrt_upsample.h", "vrt_reproject_cam.h", "vrt_reproject.h", "vrt_raygen.h", "vrt_spec.h")]

MODELS = ("perspective", "orthographic", "panorama")
MODEL_ID = {"perspective": ref.PERSPECTIVE, "orthographic": ref.ORTHOGRAPHIC, "panorama": ref.PANORAMA}
SIZES = [(24, 14, 48, 28), (37, 21, 64, 36), (9, 5, 9, 5), (1, 1, 3, 2)]
SEAM = (32, 16, 64, 32)
FRAMES = 5
FOV_DEG = 70.0
HALF_WIDTH = 14.0
N = 40
ROOM_AT = (19.3, 20.2, 18.7)
# the seam test's offsets, in render pixels: at a ratio of 2 a sample of render column 0 pushed left by more than half a pixel falls
# left of display position -0.5, that is past the seam, within one display pixel of column 0 the short way round
SEAM_OFFSETS = ((-0.6, 0.2), (0.6, -0.2), (-0.7, 0.1), (0.3, 0.3))

_lib = None


def host():
    """The host build of csrc/vrt_upsample_cam.h and camera_ray_offset, as a ctypes library."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB) or any(os.path.getmtime(LIB) < os.path.getmtime(p) for p in DEPS):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", LIB, SRC])
        l = C.CDLL(LIB)
        l.uch_upsample.restype = C.c_int
        l.uch_upsample.argtypes = [C.c_int] * 4 + [C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_float] + [C.c_void_p] * 9
        l.uch_default_tol_rel.restype = C.c_float
        l.uch_default_tol_rel.argtypes = [C.c_void_p, C.c_int]
        l.uch_rays_offset.restype = C.c_int
        l.uch_rays_offset.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p]
        l.uch_project.restype = C.c_int
        l.uch_project.argtypes = [C.c_void_p] + [C.c_int] * 5 + [C.c_void_p] * 3
        l.uch_sizeof_camera.restype = C.c_size_t
        _lib = l
    return _lib


def host_upsample(w, h, TW, TH, cur, prev, color8, position, normal8, hist=None, max_history=32, tol_abs=0.5, tol_rel=None):
    """csrc/vrt_upsample_cam.h over host planes; (code, the result in the reference's layout)."""
    l = host()
    c = np.ascontiguousarray(color8, np.uint8); p = np.ascontiguousarray(position, np.float32); n = np.ascontiguousarray(normal8, np.int8)
    if tol_rel is None:
        tol_rel = l.uch_default_tol_rel(C.byref(cur), w)
    out = {"color16": np.zeros((TH, TW, 4), np.uint16), "surface": np.zeros((TH, TW, 4), np.uint32),
           "resolved8": np.zeros((TH, TW, 4), np.uint8), "motion": np.zeros((TH, TW, 2), np.float32)}
    hc = np.ascontiguousarray(hist[0], np.uint16) if hist is not None else None
    hs = np.ascontiguousarray(hist[1], np.uint32) if hist is not None else None
    ptr = lambda a: a.ctypes.data if a is not None else None
    r = l.uch_upsample(w, h, TW, TH, C.byref(cur), C.byref(prev), max_history, tol_abs, tol_rel, ptr(c), ptr(p), ptr(n), ptr(hc), ptr(hs),
                       ptr(out["color16"]), ptr(out["surface"]), ptr(out["resolved8"]), ptr(out["motion"]))
    return r, out


def host_rays_offset(cam, W, H, offset):
    o = np.zeros((W * H, 3), np.float32); d = np.zeros((W * H, 3), np.float32)
    r = host().uch_rays_offset(C.byref(cam), W, H, float(offset[0]), float(offset[1]), o.ctypes.data, d.ctypes.data)
    return r, o, d


def host_project(cam, w, h, TW, TH, P):
    """The header's projection of world points P [..., 3] through cam: (code, front bool [...], x, y float32 [...])."""
    pts = np.ascontiguousarray(P, np.float32).reshape(-1, 3)
    front = np.zeros(len(pts), np.uint8); xy = np.zeros((len(pts), 2), np.float32)
    r = host().uch_project(C.byref(cam), w, h, TW, TH, len(pts), pts.ctypes.data, front.ctypes.data, xy.ctypes.data)
    shape = np.shape(P)[:-1]
    return r, front.astype(bool).reshape(shape), xy[:, 0].reshape(shape), xy[:, 1].reshape(shape)


def room():
    """[z, y, x] ids of the closed room: walls one voxel thick on all six sides, and blocks of other materials on the floor."""
    vol = np.zeros((N, N, N), np.uint8)
    vol[0], vol[-1], vol[:, 0], vol[:, -1], vol[:, :, 0], vol[:, :, -1] = 3, 4, 5, 6, 7, 8
    rng = np.random.RandomState(5)
    for k in range(14):
        x, z = rng.randint(3, N - 8, 2)
        if abs(x - ROOM_AT[0]) < 6 and abs(z - ROOM_AT[2]) < 6:
            continue
        s, t = rng.randint(2, 6), rng.randint(4, 16)
        vol[z:z + s, N - 1 - t:N - 1, x:x + s] = 20 + k
    return vol


def volume_of(vrt, model):
    return room() if model == "panorama" else rc.scene_of(vrt, 1)[0]


def jitter_of(vrt, w, TW, index):
    lib = vrt.lib()
    phases = int(lib.vrt_jitter_phase_count(w, TW))
    jx, jy = C.c_float(), C.c_float()
    assert lib.vrt_jitter_offset(index % phases, phases, C.byref(jx), C.byref(jy)) == 0
    return jx.value, jy.value


def sequence(vrt, oracle, model, w, h, TW, frames=FRAMES, moving=True, offsets=True, slide=0.0, offset_list=None):
    """(pass cameras, ray cameras, offsets) frame by frame: the pass camera carries neither jitter nor offset; the perspective
    model's ray camera has the frame's vrt_jitter_offset as camera_jitter and offset (0, 0), the other two models' ray camera is
    the pass camera and the same values are the offset.  moving=False: the first pose throughout; offset_list: those instead of vrt_jitter_offset's.
    A panorama moves through the room; slide != 0 is its step along z per frame, which carries the surfaces in direction -x across
    the seam (a panorama has no yaw)."""
    cap = vrt._capi
    pushes = rc.pushes_of(vrt, oracle, w, h, frames, jittered=False)
    cams, raycams, offs = [], [], []
    for f in range(frames):
        g = f if moving else 0
        j = jitter_of(vrt, w, TW, f) if offsets else (0.0, 0.0)
        if offset_list is not None:
            j = tuple(float(v) for v in offset_list[f])
        if model == "panorama":
            at = (ROOM_AT[0] + 0.35 * g, ROOM_AT[1] - 0.2 * g, ROOM_AT[2] + (slide if slide else 0.3) * g)
            c = vrt.RayCamera.panorama(at).to_c((w, h))
        else:
            c = cap.RayCamera()
            c.model = MODEL_ID[model]
            c.basis = cap.Push.from_buffer_copy(pushes[g])
            c.tan_half = float(np.float32(np.tan(np.radians(FOV_DEG) / 2.0)))
            c.half_width = HALF_WIDTH
        rcam = cap.RayCamera.from_buffer_copy(c)
        if model == "perspective":
            rcam.basis.camera_jitter[:] = [j[0], j[1]]
            j = (0.0, 0.0)
        cams.append(c); raycams.append(rcam); offs.append(j)
    return cams, raycams, offs


def colour_of(mat, w, h, f):
    """A pattern of the material, the pixel and the frame: it changes from frame to frame, which is all the blend needs."""
    idx = np.arange(h * w, dtype=np.uint32)
    col = np.zeros((h * w, 4), np.uint8)
    for ch in range(3):
        col[:, ch] = ((mat * (37 + 20 * ch) + idx * (3 + ch) + (f + 1) * (41 + 7 * ch)) % 256).astype(np.uint8)
    return col.reshape(h, w, 4)


def trace(oracle, osn, o, d, w, h):
    """(position float32 [h, w, 4], normal8 int8 [h, w, 4], material uint32 [h * w]) of the rays, as the geometry stage writes them."""
    pos = np.zeros((h * w, 4), np.float32); nrm = np.zeros((h * w, 4), np.int8); mat = np.zeros(h * w, np.uint32)
    for i in range(h * w):
        hit = oracle.trace_ray(osn, o[i], d[i], 512)
        if hit.material:
            pos[i, :3] = hit.pos[:]
            nrm[i, :3] = [int(np.floor(v * 127.0 + 0.5)) for v in hit.normal]
            mat[i] = hit.material
    return pos.reshape(h, w, 4), nrm.reshape(h, w, 4), mat


def oracle_frames(vrt, oracle, vol, raycams, offs, w, h, shade=None):
    """[(color8, position, normal8)] of the sequence: every ray of upsample_cam_reference.camera_rays_offset traced by the oracle.
    shade: a wave number; the colour is then surface_colour of the G-buffer, the same in every frame (what the convergence test
    compares images by)."""
    osn = oracle.OracleScene(vol, vrt.synthetic.default_palette())
    out = []
    for f, (cam, off) in enumerate(zip(raycams, offs)):
        o, d = ref.camera_rays_offset(cam, w, h, off)
        pos, nrm, mat = trace(oracle, osn, o, d, w, h)
        col = surface_colour(pos, nrm, shade) if shade is not None else colour_of(mat, w, h, f)
        out.append((col, pos, nrm))
    return out


def surface_colour(pos, nrm, k):
    """A shading of the G-buffer alone: per channel a wave of wave number k (radians per voxel) along the surface, brighter on faces
    that look up or along -z; 0 on a miss.  Smooth on a face, so a display-resolution image holds detail a render-resolution one
    cannot."""
    hit = (nrm[..., :3] != 0).any(axis=-1)
    s = pos[..., 0].astype(np.float64) + 0.7 * pos[..., 1] + 1.3 * pos[..., 2]
    face = 0.75 + 0.25 * (nrm[..., 1].astype(np.float64) - nrm[..., 2]) / 127.0 / 2.0
    col = np.zeros(pos.shape[:2] + (4,), np.uint8)
    for ch in range(3):
        col[..., ch] = np.where(hit, np.floor(face * (128.0 + 100.0 * np.sin(k * s + 2.0 * ch)) + 0.5), 0).astype(np.uint8)
    return col


def run_definition(w, h, TW, TH, cams, frames, max_history=32):
    """The definition along the sequence: frame k's history feeds frame k + 1.  Returns the list of per-frame result dicts."""
    out, hist = [], None
    for k, (c, p, n) in enumerate(frames):
        r = ref.upsample(w, h, TW, TH, cams[k], cams[k - 1] if k else cams[0], c, p, n, hist, max_history)
        hist = (r["color16"], r["surface"])
        out.append(r)
    return out


_CACHE = {}


def case(vrt, oracle, model, size, **kw):
    """(cams, raycams, offsets, frames, expected) of one sequence, computed once per session."""
    key = (model, size, tuple(sorted(kw.items())))
    if key not in _CACHE:
        w, h, TW, TH = size
        cams, raycams, offs = sequence(vrt, oracle, model, w, h, TW, **kw)
        frames = oracle_frames(vrt, oracle, volume_of(vrt, model), raycams, offs, w, h)
        _CACHE[key] = (cams, raycams, offs, frames, run_definition(w, h, TW, TH, cams, frames))
    return _CACHE[key]
