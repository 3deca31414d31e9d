"""vrt_camera_rays on the GPU (csrc/vrt_rays.hip): the rays of the three camera models against the numpy restatement of
csrc/vrt_raygen.h bit for bit, the perspective model at tan_half = 1 against the renderer's own rays (vrt_pick_pixels), the rays
as input of vrt_trace_rays against the oracle, and back-to-back panorama calls on one context."""
import numpy as np
import pytest

import raygen_reference as ref
from helpers import metallic_palette
from ray_query_common import oracle_records, planes_differ
from test_gpu_ray_query import _volume

pytestmark = pytest.mark.gpu

DIMS = (64, 64, 64)
POSE = dict(pos=(31.3, 20.7, -44.1), yaw=83.0, pitch=-11.0)
# one pixel, odd sizes, one wave's 64 columns and one more, a workgroup's 4 rows and one more, two workgroups each way
SIZES = ((1, 1), (7, 5), (64, 4), (65, 5), (200, 9))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _rays(engine, cam, res, jitter=(0.0, 0.0)):
    o, d = cam.rays(engine, res, jitter)
    engine.synchronize()
    return o.cpu().numpy(), d.cpu().numpy()


def _cameras(vrt):
    ctl = vrt.CameraController(position=(31.3, 20.7, -44.1), yaw=83.0, pitch=-11.0)
    basis = dict(pos=ctl.position, cam_dir=ctl.direction, right=ctl.right, up=ctl.up)
    return [("perspective55", vrt.RayCamera.perspective(ctl, 55.0), ref.PERSPECTIVE,
             dict(basis, jitter=(0.31, -0.23), tan_half=float(np.float32(np.tan(np.radians(55.0) / 2))))),
            ("ortho", vrt.RayCamera.orthographic(ctl, 37.5), ref.ORTHOGRAPHIC, dict(basis, half_width=37.5)),
            ("panorama", vrt.RayCamera.panorama((32.5, 40.3, 20.2)), ref.PANORAMA, dict(pos=(32.5, 40.3, 20.2)))]


@pytest.mark.parametrize("res", SIZES)
def test_rays_equal_the_definition(vrt, engine, res):
    """Every ray of every model equals tests/raygen_reference.py, bit for bit, and nothing is written behind the last ray."""
    import torch
    W, H = res
    for name, cam, model, kw in _cameras(vrt):
        o, d = _rays(engine, cam, res, jitter=(0.31, -0.23))
        eo, ed = ref.camera_rays(model, W, H, **kw)
        assert o.shape == (W * H, 3) and (_bits(o) == _bits(eo)).all() and (_bits(d) == _bits(ed)).all(), (name, res)
        # into the front of larger buffers: the floats behind ray W * H - 1 keep their content
        ob = torch.full((W * H + 64, 3), 7.0, dtype=torch.float32, device=engine.torch_device); db = ob.clone()
        c = cam.to_c(res, (0.31, -0.23))
        import ctypes as C
        vrt._capi.check(vrt.lib().vrt_camera_rays(engine.ctx, C.byref(c), W, H, C.c_void_p(ob.data_ptr()), C.c_void_p(db.data_ptr())))
        engine.synchronize()
        ob, db = ob.cpu().numpy(), db.cpu().numpy()
        assert (_bits(ob[:W * H]) == _bits(eo)).all() and (_bits(db[:W * H]) == _bits(ed)).all(), (name, res)
        assert (ob[W * H:] == 7.0).all() and (db[W * H:] == 7.0).all(), (name, res)


def test_perspective_at_90_degrees_is_the_renderers_camera(vrt, oracle, engine):
    """RayCamera.perspective(90) with jitter equals oracle.primary_ray at every pixel of a 200x120 frame, and tracing those rays
    gives the records vrt_pick_pixels gives for the same push: the generator is the geometry stage's ray."""
    N, res = 128, (200, 120)
    W, H = res
    sc = vrt.VoxelScene.from_dense(engine, vrt.synthetic.treehouse(N, seed=2), metallic_palette(vrt))
    pos, yaw, pitch = vrt.synthetic.default_camera_for(N, N, N)
    ctl = vrt.CameraController(position=pos, yaw=yaw, pitch=pitch)
    push = vrt.make_push(ctl, (N, N, N), res, 3, (0.31, -0.23))
    cam = vrt.RayCamera.perspective(ctl, 90.0)
    assert cam.tan_half == 1.0
    o, d = cam.rays(engine, res, jitter=(0.31, -0.23))
    rec = sc.trace_rays(o, d, 512)
    ys, xs = np.mgrid[0:H, 0:W]
    xy = np.stack([xs.reshape(-1), ys.reshape(-1)], axis=1).astype(np.int32)
    want = sc.pick(push, xy, 512)
    engine.synchronize()
    rec = {k: v.cpu().numpy() for k, v in rec.items()}
    assert 0.05 < (want["material"] != 0).mean() < 0.95
    assert planes_differ(rec, want).size == 0
    sub = np.random.default_rng(3).permutation(W * H)[:2000]
    rays = [oracle.primary_ray(push, int(xy[i, 0]), int(xy[i, 1])) for i in sub]
    on, dn = o.cpu().numpy(), d.cpu().numpy()
    assert (_bits(on[sub]) == _bits(np.array([r[0] for r in rays]))).all() and (_bits(dn[sub]) == _bits(np.array([r[1] for r in rays]))).all()
    sc.destroy()


def test_other_cameras_trace_like_the_oracle(vrt, oracle, engine):
    """Orthographic and panorama rays at 64x32 through vrt_trace_rays equal the oracle's vo_trace_ray of the same rays, the
    orthographic view from an oblique pose and along +z exactly; every view hits something and misses something."""
    vol = _volume()
    pal = metallic_palette(vrt)
    sc = vrt.VoxelScene.from_dense(engine, vol, pal)
    osn = oracle.OracleScene(vol, pal)
    ctl = vrt.CameraController(position=POSE["pos"], yaw=POSE["yaw"], pitch=POSE["pitch"])      # (no direction component is exactly 0)
    # ... and an orthographic view along +z exactly.  yaw = 90 does not give one (cos of the float nearest pi / 2 is -4.4e-8), so the
    # controller's basis is set to the axes themselves: the rays then have two zero direction components and, with these numbers, no
    # origin component on a face of the volume (the case include/vrt.h leaves open)
    axial = vrt.CameraController(position=(32.3, 31.7, -20.0))
    axial.normalDir = np.array([0.0, 0.0, 1.0], np.float32); axial.direction = axial.normalDir.copy()
    axial.right = np.array([1.0, 0.0, 0.0], np.float32); axial.up = np.array([0.0, -1.0, 0.0], np.float32)
    for name, cam in (("ortho", vrt.RayCamera.orthographic(ctl, 40.0)), ("panorama", vrt.RayCamera.panorama((32.5, 40.3, 20.2))),
                      ("ortho along +z", vrt.RayCamera.orthographic(axial, 40.0))):
        o, d = cam.rays(engine, (64, 32))
        if name == "ortho along +z":
            dn, on = d.cpu().numpy(), o.cpu().numpy()
            assert (dn[:, :2] == 0.0).all() and (dn[:, 2] > 0.0).all()
            assert not ((on[:, :2] == 0.0) | (on[:, :2] == 64.0)).any()
        rec = sc.trace_rays(o, d, 512)
        engine.synchronize()
        rec = {k: v.cpu().numpy() for k, v in rec.items()}
        exp, _ = oracle_records(oracle, osn, o.cpu().numpy(), d.cpu().numpy(), 512)
        assert (exp["material"] != 0).any() and (exp["material"] == 0).any(), name
        assert planes_differ(rec, exp).size == 0, name
    sc.destroy()


def test_panorama_calls_back_to_back(vrt, engine):
    """Two panoramas of different sizes enqueued without a wait between them (the second refills the context's tables) and a third
    of the first size again: each equals the definition."""
    a = vrt.RayCamera.panorama((1.0, 2.0, 3.0)); b = vrt.RayCamera.panorama((-4.0, 5.0, 6.5))
    ra = a.rays(engine, (96, 40)); rb = b.rays(engine, (33, 70)); rc = a.rays(engine, (96, 40))
    engine.synchronize()
    for (o, d), (W, H), pos in ((ra, (96, 40), (1.0, 2.0, 3.0)), (rb, (33, 70), (-4.0, 5.0, 6.5)), (rc, (96, 40), (1.0, 2.0, 3.0))):
        eo, ed = ref.camera_rays(ref.PANORAMA, W, H, pos=pos)
        assert (_bits(o.cpu().numpy()) == _bits(eo)).all() and (_bits(d.cpu().numpy()) == _bits(ed)).all(), (W, H)
