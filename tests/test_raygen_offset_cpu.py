"""Ray generation with a sub-pixel offset without a GPU: camera_ray_offset / panorama_tables_offset (csrc/vrt_raygen.h, compiled for
the host by tests/native/upsample_cam_host.cpp) against the numpy restatement (tests/upsample_cam_reference.py) bit for bit, offset
(0, 0) against vrt_camera_rays' definition (tests/raygen_reference.py), where an offset ray's hit point lands under
vrt_upsample_camera's projection, and the argument errors of vrt_camera_rays_offset."""
import ctypes as C

import numpy as np
import pytest

import raygen_reference as rays
import upsample_cam_common as uc
import upsample_cam_reference as ref

SIZES = ((1, 1), (7, 5), (64, 33))
OFFSETS = ((0.0, 0.0), (0.31, -0.23), (-0.5, 0.5), (1.0, -1.0))


def _cam(vrt, model, res, jitter=(0.0, 0.0)):
    c = vrt._capi.RayCamera()
    c.model = model
    c.basis = vrt.make_push(vrt.CameraController(position=(12.3, 20.2, -6.0), yaw=80.0, pitch=7.0), (40, 40, 40), res, 0, jitter)
    c.tan_half, c.half_width = float(np.float32(np.tan(np.radians(35.0)))), 14.0
    return c


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("model", (ref.PERSPECTIVE, ref.ORTHOGRAPHIC, ref.PANORAMA))
def test_header_matches_numpy(vrt, model, W, H, offset):
    cam = _cam(vrt, model, (W, H), jitter=(0.3, -0.2))
    r, o, d = uc.host_rays_offset(cam, W, H, offset)
    eo, ed = ref.camera_rays_offset(cam, W, H, offset)
    assert r == 0 and (_bits(o) == _bits(eo)).all() and (_bits(d) == _bits(ed)).all()
    if offset == (0.0, 0.0):
        # vrt_camera_rays' rays bit for bit, the perspective model's non-zero camera_jitter included
        b = cam.basis
        zo, zd = rays.camera_rays(model, W, H, list(b.cam_pos)[:3], list(b.cam_dir)[:3], list(b.cam_right)[:3], list(b.cam_up)[:3],
                                  list(b.camera_jitter), cam.tan_half, cam.half_width)
        assert (_bits(o) == _bits(zo)).all() and (_bits(d) == _bits(zd)).all()
    elif W > 1:
        assert (_bits(d) != _bits(ref.camera_rays_offset(cam, W, H, (0.0, 0.0))[1])).any() or model == ref.ORTHOGRAPHIC


# The largest deviation, in display pixels, of a projected hit point from ((px + 0.5 + ox) TW / w - 0.5, (py + 0.5 + oy) TH / h - 0.5)
# over this test's rays, measured on the numpy reference (hit points 5 and 30 voxels along the rays).  Orthographic: 1.68e-5, fp32
# rounding.  Panorama: 2.7e-5 for every sample that stays on its side of the seam, and 0.0376 for the samples of the last column
# pushed across it by ox = 1 at TW = 109: the period of the rays is 1 / 0.1591f = 6.2854 rad, that of the projection's atan2 is
# 2 pi, and the 0.0022 rad between them (vrt_reproject_cam.h) are 0.0022 * 0.1591 * TW = 3.5e-4 TW display pixels.  Below the 1/16
# display pixel that the tent's weights in 1/256 can tell apart at this test's sizes, and it passes 1/16 at TW > 178.  It is NOT
# confined to samples that leave their pixel: every sample with (px + 0.5 + ox) / w within 1.73e-4 of 0 or 1 has an azimuth past
# +-pi and is misplaced alike -- for column 0 that is 0.5 + ox < 1.73e-4 w, which vrt_jitter_offset's values never reach at
# w < 180 (hence not at this test's w <= 64) but reach in 11 of the 32 phases at 960 -> 1920 (0.663 display pixel, measured with
# the header's projection).  Open: DESIGN.md 8.  The rays and the projection here are the HEADER's (uc.host_rays_offset,
# uc.host_project), held to the numpy reference bit for bit on the way.  The bound asserted is twice the measured value.
MEASURED = {ref.ORTHOGRAPHIC: 1.68e-5, ref.PANORAMA: 0.0376}


@pytest.mark.parametrize("model", (ref.ORTHOGRAPHIC, ref.PANORAMA))
def test_offset_rays_land_where_the_pass_projects_them(vrt, model):
    worst = 0.0
    for (w, h, TW, TH) in ((7, 5, 14, 10), (64, 33, 109, 56), (32, 16, 64, 32)):
        cam = _cam(vrt, model, (w, h))
        for off in OFFSETS[1:] + ((-0.6, 0.2),):
            r, o, d = uc.host_rays_offset(cam, w, h, off)                       # the header's rays, and below its projection
            eo, ed = ref.camera_rays_offset(cam, w, h, off)
            assert r == 0 and (_bits(o) == _bits(eo)).all() and (_bits(d) == _bits(ed)).all()
            py, px = np.mgrid[0:h, 0:w]
            for t in (5.0, 30.0):
                P = (o + np.float32(t) * d).astype(np.float32).reshape(h, w, 3)
                r, front, x, y = uc.host_project(cam, w, h, TW, TH, P)
                ef, ex, ey = ref.project(w, h, TW, TH, cam, P)
                assert r == 0 and front.all() and ef.all() and (_bits(x) == _bits(ex)).all() and (_bits(y) == _bits(ey)).all()
                wx = (px + 0.5 + np.float32(off[0])) * TW / w - 0.5
                wy = (py + 0.5 + np.float32(off[1])) * TH / h - 0.5
                dx = np.abs(x.astype(np.float64) - wx)
                if model == ref.PANORAMA:
                    dx = np.minimum(dx, np.abs(TW - dx))                       # one period in x
                    ok = (wy > -0.5) & (wy < TH - 0.5)                         # a row pushed past a pole comes back on the other side
                else:
                    ok = np.ones_like(dx, bool)
                worst = max(worst, float(dx[ok].max()), float(np.abs(y.astype(np.float64) - wy)[ok].max()))
    print(f"\nmodel {model}: largest deviation {worst:.3g} display pixels")
    assert worst <= 2 * MEASURED[model] and worst < 1.0 / 16.0


def test_argument_errors(vrt):
    """Every VRT_ERR_INVALID of vrt_camera_rays_offset is answered before a context or a device is looked at, under its name."""
    lib = vrt.lib()
    W, H = 16, 8
    buf = (C.c_uint8 * (W * H * 24 + 64))()
    base = (C.addressof(buf) + 63) & ~63
    o, d = base, base + W * H * 12
    cam = _cam(vrt, ref.PERSPECTIVE, (W, H))
    off = lambda x, y: (C.c_float * 2)(x, y)

    def call(ctx=C.c_void_p(base), cam=cam, W=W, H=H, offset=off(0.25, -0.25), o=o, d=d):
        rc_ = lib.vrt_camera_rays_offset(ctx, C.byref(cam) if cam is not None else None, W, H, offset, o, d)
        return int(rc_), lib.vrt_last_error().decode()

    nan, inf = float("nan"), float("inf")
    for kw, word in ((dict(offset=None), "NULL"), (dict(offset=off(nan, 0)), "offset"), (dict(offset=off(0, inf)), "offset"),
                     (dict(offset=off(1.001, 0)), "offset"), (dict(offset=off(0, -1.5)), "offset"),
                     (dict(ctx=None), "NULL"), (dict(cam=None), "NULL"), (dict(o=None), "NULL"), (dict(d=None), "NULL"),
                     (dict(W=0), "size"), (dict(H=40000), "size"), (dict(W=16384, H=16384), "2^28"),
                     (dict(cam=_cam(vrt, 3, (W, H))), "model"), (dict(o=o + 2), "aligned"), (dict(d=o + 12), "overlap")):
        code, msg = call(**kw)
        assert code == 1 and word in msg and msg.startswith("vrt_camera_rays_offset:"), (kw, msg)
    bad = _cam(vrt, ref.PERSPECTIVE, (W, H)); bad.tan_half = 0.0
    assert "tan_half" in call(cam=bad)[1]
    bad = _cam(vrt, ref.ORTHOGRAPHIC, (W, H)); bad.half_width = nan
    assert "half_width" in call(cam=bad)[1]
    bad = _cam(vrt, ref.PANORAMA, (W, H)); bad.basis.cam_pos[1] = inf
    assert "degenerate" in call(cam=bad)[1]
    # the same broken call gives vrt_camera_rays' code and, but for the name, its message
    for kw in (dict(W=0), dict(o=o + 2), dict(d=o + 12)):
        a = dict(ctx=C.c_void_p(base), cam=cam, W=W, H=H, o=o, d=d); a.update(kw)
        rc_ = lib.vrt_camera_rays(a["ctx"], C.byref(a["cam"]), a["W"], a["H"], a["o"], a["d"])
        m0 = lib.vrt_last_error().decode()
        code, msg = call(**kw)
        assert code == rc_ and msg == m0.replace("vrt_camera_rays:", "vrt_camera_rays_offset:")
    # |o| == 1 is allowed: the next rule speaks (never a valid call here: the context is fake)
    assert "NULL" in call(offset=off(1.0, -1.0), o=None)[1]
