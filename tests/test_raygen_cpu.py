"""Ray generation (vrt_camera_rays) without a GPU: the definition (csrc/vrt_raygen.h, run by the program
tests/native/raygen_host.cpp) against its numpy float32 restatement (tests/raygen_reference.py) and against the oracle's
vo_primary_ray bit for bit, the panorama's unit length, the same program under ASan + UBSan, and the argument checks of
vrt_camera_rays that are made before a context or a device is looked at."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import raygen_reference as ref
from helpers import camera_push

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "raygen_host.cpp")
SIZES = ((1, 1), (7, 5), (64, 33))
INVALID = 1


def _build(tmp_path_factory, name, flags):
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall"] + flags + ["-o", exe, SRC])
    return exe


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return _build(tmp_path_factory, "raygen_host", ["-O2"])


@pytest.fixture(scope="module")
def prog_san(tmp_path_factory):
    """The same program with AddressSanitizer and UndefinedBehaviorSanitizer: a program of its own, nothing loaded into Python."""
    return _build(tmp_path_factory, "raygen_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def camera_c(vrt, model, push, tan_half=1.0, half_width=1.0):
    c = vrt._capi.RayCamera()
    c.model, c.basis, c.tan_half, c.half_width = model, push, tan_half, half_width
    return c


def run_host(exe, tmp_path, records):
    """records: [(vrt_ray_camera, W, H)] -> [(rc, origins, dirs)]"""
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        for cam, W, H in records:
            f.write(bytes(cam)); f.write(struct.pack("<2i", W, H))
    r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    blob, o, out = open(outp, "rb").read(), 0, []
    for _, W, H in records:
        rc = struct.unpack_from("<i", blob, o)[0]; o += 4
        if rc != 0:
            out.append((rc, None, None)); continue
        n = W * H * 3
        og = np.frombuffer(blob, "<f4", n, o).reshape(-1, 3); o += 4 * n
        dr = np.frombuffer(blob, "<f4", n, o).reshape(-1, 3); o += 4 * n
        out.append((rc, og, dr))
    assert o == len(blob)
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


POSES = [dict(pos=(31.3, 20.7, -44.1), yaw=83.0, pitch=-11.0), dict(pos=(-20.5, 70.25, 12.0), yaw=-31.0, pitch=27.0)]


def _cases(vrt):
    """(name, model, camera kwargs for the reference, vrt_ray_camera maker) with non-zero jitter"""
    jit = (0.31, -0.23)
    out = []
    for k, pose in enumerate(POSES):
        ctl = vrt.CameraController(position=pose["pos"], yaw=pose["yaw"], pitch=pose["pitch"])
        basis = dict(pos=ctl.position, cam_dir=ctl.direction, right=ctl.right, up=ctl.up, jitter=jit)
        th = float(np.float32(np.tan(np.radians(55.0 + 20 * k) / 2)))
        out.append((f"perspective{k}", ref.PERSPECTIVE, dict(basis, tan_half=th), ctl, jit, dict(tan_half=th)))
        out.append((f"ortho{k}", ref.ORTHOGRAPHIC, dict(basis, half_width=37.5 + k), ctl, jit, dict(half_width=37.5 + k)))
        out.append((f"panorama{k}", ref.PANORAMA, dict(pos=ctl.position), ctl, jit, {}))
    return out


def test_header_equals_numpy_restatement(vrt, prog, tmp_path):
    """All three models at 1x1, 7x5 and 64x33 with non-zero jitter, bit for bit."""
    cases = _cases(vrt)
    records, want = [], []
    for name, model, kw, ctl, jit, ck in cases:
        for W, H in SIZES:
            push = vrt.make_push(ctl, (0, 0, 0), (W, H), 0, jit)
            records.append((camera_c(vrt, model, push, **ck), W, H))
            want.append((name, W, H, ref.camera_rays(model, W, H, **kw)))
    got = run_host(prog, tmp_path, records)
    for (rc, o, d), (name, W, H, (eo, ed)) in zip(got, want):
        assert rc == 0, (name, W, H, rc)
        assert (_bits(o) == _bits(eo)).all(), (name, W, H, np.argwhere(_bits(o) != _bits(eo))[:3])
        assert (_bits(d) == _bits(ed)).all(), (name, W, H, np.argwhere(_bits(d) != _bits(ed))[:3])
    # the models differ from each other where they should (the test is not comparing constants)
    persp, ortho = got[2], got[len(SIZES) + 2]
    assert (np.ptp(persp[1], axis=0) == 0).all() and (np.ptp(persp[2], axis=0) > 0).any()
    assert (np.ptp(ortho[2], axis=0) == 0).all() and (np.ptp(ortho[1], axis=0) > 0).any()


def test_perspective_tan_half_one_is_the_reference_camera(vrt, oracle, prog, tmp_path):
    """Perspective with tan_half = 1.0f equals oracle.primary_ray at every pixel of a 33x17 frame, two poses, one with jitter."""
    W, H = 33, 17
    pushes = [camera_push(vrt, (64, 64, 64), (W, H), pos=POSES[0]["pos"], yaw=POSES[0]["yaw"], pitch=POSES[0]["pitch"]),
              camera_push(vrt, (64, 64, 64), (W, H), pos=POSES[1]["pos"], yaw=POSES[1]["yaw"], pitch=POSES[1]["pitch"], jitter=(0.31, -0.23))]
    got = run_host(prog, tmp_path, [(camera_c(vrt, ref.PERSPECTIVE, p, tan_half=1.0), W, H) for p in pushes])
    for push, (rc, o, d) in zip(pushes, got):
        assert rc == 0
        rays = [oracle.primary_ray(push, x, y) for y in range(H) for x in range(W)]
        eo = np.array([r[0] for r in rays], np.float32); ed = np.array([r[1] for r in rays], np.float32)
        assert (_bits(o) == _bits(eo)).all() and (_bits(d) == _bits(ed)).all()


def test_panorama_directions_are_unit_vectors(vrt, prog, tmp_path):
    """| |dir|^2 - 1 | <= 4 ulp of 1 (2^-23 each) for every direction of a 640x320 and a 64x33 panorama.
    (The two table entries of an angle are cos and sin rounded to fp32, 2^-24 relative each; the products and the sum add a few
    roundings more -- evaluated here in float64 from the fp32 components, so the check adds none of its own.)"""
    ctl = vrt.CameraController(position=(1.0, 2.0, 3.0))
    for W, H in ((640, 320), (64, 33)):
        push = vrt.make_push(ctl, (0, 0, 0), (W, H))
        (rc, o, d), = run_host(prog, tmp_path, [(camera_c(vrt, ref.PANORAMA, push), W, H)])
        assert rc == 0 and (o == np.array([1.0, 2.0, 3.0], np.float32)).all()
        n2 = (d.astype(np.float64) ** 2).sum(axis=1)
        worst = np.abs(n2 - 1.0).max() / 2.0 ** -23
        print(f"\npanorama {W}x{H}: worst | |dir|^2 - 1 | = {worst:.3f} ulp")
        assert worst <= 4.0
        # the middle row looks along the horizon, the columns go once around
        mid = d.reshape(H, W, 3)[H // 2]
        assert np.abs(mid[:, 1]).max() < 0.06 and mid[:, 0].min() < -0.99 and mid[:, 0].max() > 0.99


def test_bad_cameras_are_refused(vrt, prog, tmp_path):
    """raygen_consts_of: unknown model 1, bad tan_half / half_width 2, degenerate basis 3."""
    ctl = vrt.CameraController()
    push = vrt.make_push(ctl, (0, 0, 0), (8, 8))
    flat = vrt._capi.Push.from_buffer_copy(push); flat.cam_up[:] = list(push.cam_right)
    nanpos = vrt._capi.Push.from_buffer_copy(push); nanpos.cam_pos[0] = float("nan")
    recs = [(camera_c(vrt, 3, push), 8, 8), (camera_c(vrt, -1, push), 8, 8),
            (camera_c(vrt, ref.PERSPECTIVE, push, tan_half=0.0), 8, 8), (camera_c(vrt, ref.PERSPECTIVE, push, tan_half=float("inf")), 8, 8),
            (camera_c(vrt, ref.PERSPECTIVE, push, tan_half=float("nan")), 8, 8), (camera_c(vrt, ref.ORTHOGRAPHIC, push, half_width=-2.0), 8, 8),
            (camera_c(vrt, ref.PERSPECTIVE, flat), 8, 8), (camera_c(vrt, ref.ORTHOGRAPHIC, flat, half_width=3.0), 8, 8),
            (camera_c(vrt, ref.PANORAMA, nanpos), 8, 8), (camera_c(vrt, ref.PANORAMA, flat), 8, 8)]
    assert [r[0] for r in run_host(prog, tmp_path, recs)] == [1, 1, 2, 2, 2, 2, 3, 3, 3, 0]


def test_sanitized_program_runs_clean(vrt, prog, prog_san, tmp_path):
    """The program built with -fsanitize=address,undefined (no recovery: any report ends it with a non-zero status) over
    every model and size of the first test, with the same output as the plain build."""
    records = []
    for name, model, kw, ctl, jit, ck in _cases(vrt):
        for W, H in SIZES:
            records.append((camera_c(vrt, model, vrt.make_push(ctl, (0, 0, 0), (W, H), 0, jit), **ck), W, H))
    a, b = run_host(prog, tmp_path, records), run_host(prog_san, tmp_path, records)
    for (ra, oa, da), (rb, ob, db) in zip(a, b):
        assert ra == rb == 0 and (_bits(oa) == _bits(ob)).all() and (_bits(da) == _bits(db)).all()


def test_c_abi_surface(vrt):
    """The symbol is exported and listed in _capi.SYMBOLS, vrt_ray_camera has the layout of its ctypes mirror, and argument errors
    come back before anything touches a context or a device (there is none here)."""
    lib = vrt.lib()
    assert "vrt_camera_rays" in vrt._capi.SYMBOLS and hasattr(C.CDLL(vrt._capi.LIB_PATH), "vrt_camera_rays")
    RC = vrt._capi.RayCamera
    assert C.sizeof(RC) == 108 and [getattr(RC, f).offset for f in ("model", "basis", "tan_half", "half_width")] == [0, 4, 100, 104]
    err = lambda: lib.vrt_last_error().decode()
    buf = (C.c_uint8 * 4096)()                     # stands for any non-NULL pointer: the calls below return before they look at it
    base = C.addressof(buf)
    base += (-base) % 16
    p = C.c_void_p(base)
    ctl = vrt.CameraController()
    cam = camera_c(vrt, ref.PERSPECTIVE, vrt.make_push(ctl, (0, 0, 0), (8, 8)))
    far = C.c_void_p(base + (1 << 20))             # a second range that does not overlap the first for an 8x8 frame
    # ---- vrt_camera_rays
    assert lib.vrt_camera_rays(None, C.byref(cam), 8, 8, p, far) == INVALID and "NULL" in err()
    assert lib.vrt_camera_rays(p, None, 8, 8, p, far) == INVALID and "NULL" in err()
    assert lib.vrt_camera_rays(p, C.byref(cam), 8, 8, None, far) == INVALID and "NULL" in err()
    assert lib.vrt_camera_rays(p, C.byref(cam), 8, 8, p, None) == INVALID and "NULL" in err()
    for W, H in ((0, 8), (8, 0), (-1, 8), (32769, 8), (16384, 16384)):
        assert lib.vrt_camera_rays(p, C.byref(cam), W, H, p, far) == INVALID and ("size" in err() or "2^28" in err()), (W, H)
    assert lib.vrt_camera_rays(p, C.byref(camera_c(vrt, 7, cam.basis)), 8, 8, p, far) == INVALID and "model" in err()
    assert lib.vrt_camera_rays(p, C.byref(camera_c(vrt, ref.PERSPECTIVE, cam.basis, tan_half=-1.0)), 8, 8, p, far) == INVALID and "tan_half" in err()
    assert lib.vrt_camera_rays(p, C.byref(camera_c(vrt, ref.ORTHOGRAPHIC, cam.basis, half_width=float("nan"))), 8, 8, p, far) == INVALID and "half_width" in err()
    flat = vrt._capi.Push.from_buffer_copy(cam.basis); flat.cam_up[:] = list(flat.cam_right)
    assert lib.vrt_camera_rays(p, C.byref(camera_c(vrt, ref.PERSPECTIVE, flat)), 8, 8, p, far) == INVALID and "degenerate" in err()
    assert lib.vrt_camera_rays(p, C.byref(cam), 8, 8, C.c_void_p(base + 2), far) == INVALID and "aligned" in err()
    assert lib.vrt_camera_rays(p, C.byref(cam), 8, 8, p, C.c_void_p(base + 8 * 8 * 12 - 4)) == INVALID and "overlap" in err()
    # the Python mirrors exist
    for m in ("perspective", "orthographic", "panorama", "rays"):
        assert callable(getattr(vrt.RayCamera, m))
    assert vrt.RayCamera.perspective(ctl, 90.0).tan_half == 1.0
