"""vrt_render_rays on the GPU (csrc/vrt_render_rays.hip): the G-buffer of caller-supplied primary rays against the oracle's main(),
every plane bit for bit, through the harness of tests/render_rays_common.py (one push block per ray under which every pixel of
the oracle's frame has that ray).  Tolerance everywhere: 0 -- the values are bits or integers."""
import ctypes as C

import numpy as np
import pytest

import render_rays_common as rr
from helpers import compare_planes, metallic_palette
from ray_query_common import bricks_of

pytestmark = pytest.mark.gpu

W, H = rr.W, rr.H
_cache = {}


def _settings(vrt, **kw):
    st = vrt.VoxelRenderSettings().to_c()            # the reference defaults: AO 4, shadows, 5 bounces, 512 steps
    for k, v in kw.items():
        setattr(st, k, v)
    return st


def _key(st):
    return (st.ao_samples, st.shadows, st.max_bounces, st.max_steps, st.ao_steps)


@pytest.fixture(scope="module")
def scene(vrt, oracle, engine):
    vol, pal, sky, noise = rr.scene_a(vrt)
    gs = vrt.VoxelScene.from_dense(engine, vol, pal, sky=sky, noise=noise)
    osn = oracle.OracleScene(vol, pal, sky=sky, noise=noise)
    return vol, gs, osn


def _raysets(vol):
    if "sets" not in _cache:
        o, p = rr.ortho_rays(), rr.panorama_rays()
        _cache["sets"] = {"orthographic": o, "panorama": p, "mixed": rr.mixed_rays(vol)}
    return _cache["sets"]


def _expected(oracle, osn, tag, rays, st, frame=rr.FRAME, w=W, h=H):
    """The oracle's frame for a ray set under settings st, computed once per (set, settings, frame) and not changed afterwards."""
    k = (tag, _key(st), frame, w, h)
    if k not in _cache:
        starts, dn, exp = rr.oracle_frame(oracle, osn, oracle.params_from(st), w, h, rays[0], rays[1], frame)
        for a in (starts, dn, *exp.values()):
            a.setflags(write=False)
        _cache[k] = (starts, dn, exp)
    return _cache[k]


def _render(vrt, engine, gs, st, w, h, origins, dirs, frame=rr.FRAME, planes=rr.ALL_PLANES):
    """vrt_render_rays into fresh planes; the result as numpy arrays (h, w, ...)."""
    import torch
    o = torch.from_numpy(np.array(origins, np.float32)).to(engine.torch_device)
    d = torch.from_numpy(np.array(dirs, np.float32)).to(engine.torch_device)
    gb = vrt.GeometryBuffer(engine, w, h, planes)
    fr = gb.to_c()
    vrt._capi.check(vrt.lib().vrt_render_rays(engine.ctx, gs.handle, w, h, C.c_void_p(o.data_ptr()), C.c_void_p(d.data_ptr()),
                                             frame, C.byref(st), C.byref(fr)))
    engine.synchronize()
    return gb.numpy()


def _check(vrt, oracle, engine, gs, osn, tag, rays, st, frame=rr.FRAME):
    starts, dn, exp = _expected(oracle, osn, tag, rays, st, frame)
    got = _render(vrt, engine, gs, st, W, H, starts, dn, frame)
    bad = compare_planes(got, exp, rr.ALL_PLANES)
    assert not bad, (tag, _key(st), bad)
    return got, exp


# ---- 2. pinhole identity (the first launch of the new kernels: the smallest and best-understood case) ------------------------------

@pytest.mark.parametrize("tan_half", [1.0, 0.5])
def test_pinhole_rays_equal_the_builtin_camera(vrt, oracle, engine, tan_half):
    """RayCamera.perspective rays (jitter (0.25, -0.4), frame 33) through record_rays == GeometryStage.record of the same push ==
    the oracle, every plane, on the 37 x 22 x 51 random scene at 45 x 37.  tan_half = 0.5: against the built-in camera with
    cam_right and cam_up halved (exact: the camera model only scales U and V)."""
    rng = np.random.default_rng(12)
    vol = (rng.random((37, 22, 51)) < 0.04).astype(np.uint8) * rng.integers(1, 256, (37, 22, 51)).astype(np.uint8)
    pal = metallic_palette(vrt, ids=range(128, 256))
    sky, noise = vrt.synthetic.sky_gradient(64, 32), vrt.synthetic.blue_noise_standin(64)
    gs = vrt.VoxelScene.from_dense(engine, vol, pal, sky=sky, noise=noise)
    osn = oracle.OracleScene(vol, pal, sky=sky, noise=noise)
    res, jitter = (45, 37), (0.25, -0.4)
    st = vrt.VoxelRenderSettings(targetResolution=res)
    st.fsrSetttings.enable = False
    ctl = vrt.CameraController(position=(25.3, 11.2, -30.0), yaw=83.0, pitch=-11.0)
    push = vrt.make_push(ctl, (51, 22, 37), res, 33, jitter)
    for a in range(3):
        push.cam_right[a] = float(np.float32(push.cam_right[a]) * np.float32(tan_half))
        push.cam_up[a] = float(np.float32(push.cam_up[a]) * np.float32(tan_half))
    cam = vrt.RayCamera(vrt._capi.CAMERA_PERSPECTIVE, ctl, tan_half=tan_half)
    names = list(rr.ALL_PLANES)
    exp = oracle.render(osn, push, oracle.params_from(st.to_c()), nthreads=8)
    assert (exp["hit_id"] != 0).mean() > 0.1 and (exp["hit_id"] == 0).mean() > 0.05
    builtin = vrt.GeometryStage(engine, st, gs, debug_planes=True).record(push)
    engine.synchronize()
    builtin = builtin.numpy()
    o, d = cam.rays(engine, res, jitter)
    got = vrt.GeometryStage(engine, st, gs, debug_planes=True).record_rays(o, d, res, frame=33)
    engine.synchronize()
    got = got.numpy()
    assert not compare_planes(got, builtin, names), compare_planes(got, builtin, names)
    assert not compare_planes(got, exp, names), compare_planes(got, exp, names)
    assert not compare_planes(builtin, exp, names)


# ---- 1. orthographic and panorama against the oracle ------------------------------------------------------------------------

@pytest.mark.parametrize("camera", ["orthographic", "panorama"])
def test_cameras_equal_the_oracle(vrt, oracle, engine, scene, camera):
    """Scene A, reference defaults, frame 3, 44 x 28: every plane of an orthographic and a panoramic view, bit for bit."""
    vol, gs, osn = scene
    st = _settings(vrt)
    got, exp = _check(vrt, oracle, engine, gs, osn, camera, _raysets(vol)[camera], st)
    hit = exp["hit_id"] != 0
    assert hit.mean() >= 0.2 and (~hit).mean() >= 0.05 and (exp["rays_total"] > 6).sum() >= 20, (hit.mean(), (exp["rays_total"] > 6).sum())


# ---- 3. a mixed frame ----------------------------------------------------------------------------------------------------------

def test_mixed_frame_equals_the_oracle(vrt, oracle, engine, scene):
    """The two cameras' rays and the edge classes (axis1, axis2, lattice_in, origins inside solid voxels) interleaved ray by ray into
    one 44 x 28 frame (render_rays_common.mixed_rays: every set subsampled so that every class lies inside the 1 232 rays):
    neighbouring lanes have nothing in common.  Asserted on the oracle's side: every class is in the frame, the three direction
    classes with hits and misses of their own, and every ray that starts inside a solid voxel is a hit with mask 0 -- rule A's zero
    normal, shaded by the shading kernel's general branch."""
    vol, gs, osn = scene
    o, d, labels = _raysets(vol)["mixed"]
    got, exp = _check(vrt, oracle, engine, gs, osn, "mixed", (o, d), _settings(vrt))
    hit = (exp["hit_id"] != 0).reshape(-1)
    mask0 = (exp["hit_mask"] == 0).reshape(-1)
    assert hit.mean() >= 0.2 and (~hit).mean() >= 0.05
    for k, name in enumerate(rr.MIXED_LABELS):
        m = labels == k
        assert m.sum() >= 64, (name, int(m.sum()))
        if name != "solid_origin":
            assert hit[m].sum() >= 10 and (~hit[m]).sum() >= 10, (name, int(hit[m].sum()), int(m.sum()))
    solid = labels == rr.MIXED_LABELS.index("solid_origin")
    assert (hit & mask0)[solid].all()
    starts = _cache[("mixed", _key(_settings(vrt)), rr.FRAME, W, H)][0]
    lat = labels == rr.MIXED_LABELS.index("lattice_in")
    assert (starts[lat] == np.floor(starts[lat])).all()                          # the origins are still on the lattice as fed


# ---- 4. settings -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,kw", [("primary_only", dict(ao_samples=0, shadows=0, max_bounces=0)),
                                     ("shadows_only", dict(ao_samples=0, shadows=1, max_bounces=0)),
                                     ("max_steps_37", dict(max_steps=37)), ("max_steps_2000", dict(max_steps=2000))])
def test_settings_equal_the_oracle(vrt, oracle, engine, scene, name, kw):
    """Scene A, orthographic rays: primary only; shadows only; a budget of 37; a budget of 2000 (VRT_TRAVERSAL_DF in both kernels)."""
    vol, gs, osn = scene
    _check(vrt, oracle, engine, gs, osn, "orthographic", _raysets(vol)["orthographic"], _settings(vrt, **kw))


def test_ao_only_with_and_without_the_pool(vrt, oracle, engine, scene):
    """AO only, context option ao_batch 0 and 1: both equal the oracle, and each other."""
    vol, gs, osn = scene
    st = _settings(vrt, shadows=0, max_bounces=0)
    outs = []
    for batch in (0, 1):
        with engine.options(ao_batch=batch):
            outs.append(_check(vrt, oracle, engine, gs, osn, "orthographic", _raysets(vol)["orthographic"], st)[0])
    assert not compare_planes(outs[0], outs[1], rr.ALL_PLANES)


# ---- 5. brick scene ----------------------------------------------------------------------------------------------------------------

def test_brick_scene_equals_the_dense_scene(vrt, oracle, engine, scene):
    """Scene A through VoxelScene.from_bricks: planes equal to the dense scene's (and so to the oracle's), bit for bit."""
    vol, gs, osn = scene
    _, pal, sky, noise = rr.scene_a(vrt)
    grid, pool = bricks_of(vol)
    bs = vrt.VoxelScene.from_bricks(engine, grid, pool, pal, sky=sky, noise=noise)
    st = _settings(vrt)
    for camera in ("orthographic", "panorama"):
        starts, dn, exp = _expected(oracle, osn, camera, _raysets(vol)[camera], st)
        dense = _render(vrt, engine, gs, st, W, H, starts, dn)
        brick = _render(vrt, engine, bs, st, W, H, starts, dn)
        assert not compare_planes(brick, dense, rr.ALL_PLANES), camera
        assert not compare_planes(brick, exp, rr.ALL_PLANES), camera


# ---- 6. all miss / all hit -------------------------------------------------------------------------------------------------------

def test_all_miss_and_all_hit(vrt, oracle, engine, scene):
    """The panorama from (-40, -40, -40): by the oracle 7 of its 1 232 rays still meet the volume (a panorama looks every way), so
    beside it the orthographic rays turned round (direction negated: they leave the volume behind them) are the frame in which no
    ray hits and every shading workgroup leaves.  An orthographic view with half_width 4 into a solid 16^3 block: every ray hits."""
    vol, gs, osn = scene
    st = _settings(vrt)
    far = rr.panorama_rays(at=(-40.0, -40.0, -40.0))
    got, exp = _check(vrt, oracle, engine, gs, osn, "panorama_far", far, st)
    assert (exp["hit_id"] != 0).sum() <= 16
    away = rr.ortho_rays(cam_dir=tuple(-c for c in rr.ORTHO["cam_dir"]))
    got, exp = _check(vrt, oracle, engine, gs, osn, "ortho_away", away, st)
    assert (exp["hit_id"] == 0).all() and (got["mask8"] == 0).all()
    block = np.full((16, 16, 16), 201, np.uint8)
    block[:, :, ::2] = 7                                        # metallic and plain columns
    pal = metallic_palette(vrt)
    sky, noise = vrt.synthetic.sky_gradient(64, 32), vrt.synthetic.blue_noise_standin(64)
    bgs = vrt.VoxelScene.from_dense(engine, block, pal, sky=sky, noise=noise)
    bosn = oracle.OracleScene(block, pal, sky=sky, noise=noise)
    rays = rr.ortho_rays(pos=(8.1, 7.9, -6.0), cam_dir=(0.05, 0.02, 1.0), right=(1.0, 0.0, -0.05), up=(0.0, -1.0, 0.02), half_width=4.0)
    got, exp = _check(vrt, oracle, engine, bgs, bosn, "block", rays, st)
    assert (exp["hit_id"] != 0).all() and (got["mask8"] == 230).all()


# ---- 7. plane subsets and bounds -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("subset", [("color8",), ("depth", "position")])
def test_plane_subsets_and_guards(vrt, oracle, engine, scene, subset):
    """Only some planes attached, every plane allocated with 4 096 guard bytes of 0xA5 on both sides: the attached planes equal the
    oracle, the guards are intact, the planes that were not attached are not written."""
    import torch
    vol, gs, osn = scene
    st = _settings(vrt)
    starts, dn, exp = _expected(oracle, osn, "orthographic", _raysets(vol)["orthographic"], st)
    G = 4096
    bpp = {"color8": 4, "depth": 4, "motion": 8, "mask8": 1, "position": 16, "normal8": 4, "color_f": 12, "hit_id": 1, "hit_voxel": 6, "hit_mask": 1}
    bufs = {n: torch.full((G + W * H * b + G,), 0xA5, dtype=torch.uint8, device=engine.torch_device) for n, b in bpp.items()}
    o = torch.from_numpy(starts.copy()).to(engine.torch_device); d = torch.from_numpy(dn.copy()).to(engine.torch_device)
    fr = vrt._capi.Frame()
    for n in subset:
        setattr(fr, n, bufs[n].data_ptr() + G)
    vrt._capi.check(vrt.lib().vrt_render_rays(engine.ctx, gs.handle, W, H, C.c_void_p(o.data_ptr()), C.c_void_p(d.data_ptr()),
                                             rr.FRAME, C.byref(st), C.byref(fr)))
    engine.synchronize()
    for n, b in bpp.items():
        raw = bufs[n].cpu().numpy()
        assert (raw[:G] == 0xA5).all() and (raw[-G:] == 0xA5).all(), n
        body = raw[G:-G]
        if n in subset:
            assert body.tobytes() == np.ascontiguousarray(exp[n]).tobytes(), n
        else:
            assert (body == 0xA5).all(), n


# ---- 8. end to end ---------------------------------------------------------------------------------------------------------------

def test_panorama_through_the_denoiser_and_the_renderer(vrt, oracle, engine, scene):
    """The panorama's G-buffer through vrt_denoise (2 passes, canonical) == oracle.denoise of the oracle's planes, and
    VoxelRenderer(camera=RayCamera.panorama(...)) produces the same image."""
    vol, gs, osn = scene
    st = vrt.VoxelRenderSettings(targetResolution=(W, H))
    st.fsrSetttings.enable = False
    cam = vrt.RayCamera.panorama(rr.PANORAMA_AT)
    o, d = cam.rays(engine, (W, H))
    engine.synchronize()
    # (the camera's unit directions, not the oracle's renormalisation of them: what the renderer feeds)
    starts, dn, exp = _expected(oracle, osn, "panorama_frame0", rr.panorama_rays(), st.to_c(), frame=0)
    eimg = oracle.denoise(exp["color8"], exp["normal8"], exp["position"])
    stage = vrt.GeometryStage(engine, st, gs)
    import torch
    gb = stage.record_rays(torch.from_numpy(starts.copy()).to(engine.torch_device), torch.from_numpy(dn.copy()).to(engine.torch_device), (W, H), frame=0)
    img = vrt.DenoiserStage(engine, st).record(gb.color, gb.normal, gb.position)
    engine.synchronize()
    assert (img.cpu().numpy() == eimg).all()
    r = vrt.VoxelRenderer(engine, st, gs, camera=cam)
    rimg = r.render()
    engine.synchronize()
    # the renderer's rays are the camera's own; where the oracle's renormalisation left a direction unchanged the pixels are the oracle's
    same = (d.cpu().numpy().view(np.uint32) == dn.view(np.uint32)).all(axis=1).reshape(H, W)
    assert same.mean() > 0.5
    g = r.gBuffer.numpy()
    for n in rr.GB_PLANES:
        assert (g[n][same] == exp[n][same]).all(), n
    own = _render(vrt, engine, gs, st.to_c(), W, H, o.cpu().numpy(), d.cpu().numpy(), frame=0, planes=rr.GB_PLANES)
    assert (rimg.cpu().numpy() == oracle.denoise(own["color8"], own["normal8"], own["position"])).all()
    with pytest.raises(ValueError):
        vrt.VoxelRenderer(engine, st, gs, camera=cam, temporal=True)


def _ortho_exp(oracle, osn, push, half_width, st_c, tag):
    """The orthographic frame of a push block's basis by the oracle, or None where the oracle's renormalisation would change the
    view's one direction (then the pose cannot be compared pixel by pixel, whatever the code under test does)."""
    import raygen_reference as ref
    w, h = push.screen_size[0], push.screen_size[1]
    o, d = ref.camera_rays(ref.ORTHOGRAPHIC, w, h, pos=list(push.cam_pos)[:3], cam_dir=list(push.cam_dir)[:3], right=list(push.cam_right)[:3],
                           up=list(push.cam_up)[:3], half_width=half_width)
    _, d1 = oracle.primary_ray(rr.pixel_push(oracle, osn.dims, w, h, o[0], d[0], push.frame), 0, 0)
    if not (d1.view(np.uint32) == d[0].view(np.uint32)).all():
        return None
    starts, dn, exp = _expected(oracle, osn, tag, (o, d), st_c, frame=push.frame, w=w, h=h)
    assert (starts.view(np.uint32) == o.view(np.uint32)).all() and (dn.view(np.uint32) == d.view(np.uint32)).all()
    return exp


POSES = ((80.0, -6.0), (83.0, -6.0), (77.0, -4.0), (86.0, -9.0), (90.0, 0.0))


def test_renderer_with_an_orthographic_camera_equals_the_oracle(vrt, oracle, engine, scene):
    """VoxelRenderer(camera=RayCamera.orthographic(...)): the G-buffer equals the oracle's at every pixel and the image equals
    oracle.denoise of the oracle's planes -- an independent reference for the whole renderer path (an orthographic view has one
    direction, which the oracle's renormalisation leaves unchanged for the pose used; the poses are tried in turn until one does)."""
    vol, gs, osn = scene
    st = vrt.VoxelRenderSettings(targetResolution=(W, H))
    st.fsrSetttings.enable = False
    for yaw, pitch in POSES:
        ctl = vrt.CameraController(position=(16.3, 15.2, -10.0), yaw=yaw, pitch=pitch)
        push = vrt.make_push(ctl, osn.dims, (W, H), 0)
        exp = _ortho_exp(oracle, osn, push, 20.0, st.to_c(), ("renderer_ortho", yaw, pitch))
        if exp is not None:
            break
    assert exp is not None
    assert (exp["hit_id"] != 0).mean() >= 0.2 and (exp["hit_id"] == 0).mean() >= 0.05
    r = vrt.VoxelRenderer(engine, st, gs, camera=vrt.RayCamera.orthographic(ctl, 20.0))
    img = r.render()
    engine.synchronize()
    assert not compare_planes(r.gBuffer.numpy(), exp, rr.GB_PLANES)
    assert (img.cpu().numpy() == oracle.denoise(exp["color8"], exp["normal8"], exp["position"])).all()


def test_cpp_app_projection_equals_the_oracle(vrt, oracle, scene, tmp_path):
    """The C++ mirror: vrt_app --projection ortho:20 (GeometryStage::recordRays under VoxelRenderer::projection) writes the image the
    oracle makes of the rays of the push block the app itself computed; --projection with --temporal is refused."""
    import os
    import subprocess
    from test_gpu_cpp_host import APP, _write_dense
    assert os.path.exists(APP), "build with __graft_entry__.build()"
    vol, gs, osn = scene
    _, pal, sky, noise = rr.scene_a(vrt)
    dense = tmp_path / "scene.vrtd"
    _write_dense(dense, vol, pal, sky, noise)
    raw, pushf = tmp_path / "out.rgba", tmp_path / "push.bin"
    st = vrt.VoxelRenderSettings(targetResolution=(W, H))
    st.fsrSetttings.enable = False
    base = [APP, "--dense", str(dense), "--width", str(W), "--height", str(H), "--no-fsr", "--pos", "16.3", "15.2", "-10"]
    exp = None
    for yaw, pitch in POSES:
        r = subprocess.run(base + ["--yaw", str(yaw), "--pitch", str(pitch), "--projection", "ortho:20", "--raw", str(raw), "--dump-push", str(pushf)],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        push = oracle.Push.from_buffer_copy(pushf.read_bytes())
        assert (push.screen_size[0], push.screen_size[1], push.frame) == (W, H, 0)
        exp = _ortho_exp(oracle, osn, push, 20.0, st.to_c(), ("app_ortho", yaw, pitch))
        if exp is not None:
            break
    assert exp is not None
    assert (exp["hit_id"] != 0).mean() >= 0.2 and (exp["hit_id"] == 0).mean() >= 0.05
    got = np.frombuffer(raw.read_bytes(), np.uint8).reshape(H, W, 4)
    assert (got == oracle.denoise(exp["color8"], exp["normal8"], exp["position"])).all()
    r = subprocess.run(base + ["--projection", "panorama", "--temporal", "--raw", str(raw)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "--projection" in r.stderr
    r = subprocess.run(base + ["--projection", "fisheye", "--raw", str(raw)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "--projection" in r.stderr


# ---- 9. refusals -----------------------------------------------------------------------------------------------------------------

def test_refusals(vrt, oracle, engine, scene):
    """Every VRT_ERR_INVALID and VRT_ERR_UNSUPPORTED case, with vrt_last_error naming the function; a good call on the same context
    afterwards is still correct."""
    import torch
    vol, gs, osn = scene
    lib, capi = vrt.lib(), vrt._capi
    st = _settings(vrt)
    starts, dn, exp = _expected(oracle, osn, "orthographic", _raysets(vol)["orthographic"], st)
    n = W * H
    o = torch.from_numpy(starts.copy()).to(engine.torch_device); d = torch.from_numpy(dn.copy()).to(engine.torch_device)
    gb = vrt.GeometryBuffer(engine, W, H, rr.ALL_PLANES + ("steps_primary", "steps_total", "rays_total", "color8_strips"))
    good = gb.to_c(only=rr.ALL_PLANES)

    def call(ctx=engine.ctx, sc=gs.handle, w=W, h=H, po=o.data_ptr(), pd=d.data_ptr(), s=st, f=good):
        return lib.vrt_render_rays(ctx, sc, w, h, C.c_void_p(po), C.c_void_p(pd), rr.FRAME,
                                   C.byref(s) if s is not None else None, C.byref(f) if f is not None else None)

    def refused(code, **kw):
        assert call(**kw) == code, kw
        assert b"vrt_render_rays" in lib.vrt_last_error(), lib.vrt_last_error()

    INVALID, UNSUPPORTED = 1, 7
    for kw in (dict(ctx=None), dict(sc=None), dict(po=None), dict(pd=None), dict(s=None), dict(f=None)):
        refused(INVALID, **kw)
    for kw in (dict(w=0), dict(h=0), dict(w=-3), dict(w=32769), dict(h=40000), dict(w=16384, h=16384)):
        refused(INVALID, **kw)
    refused(INVALID, s=_settings(vrt, max_steps=0))
    refused(INVALID, s=_settings(vrt, max_bounces=capi.MAX_BOUNCES + 1))
    refused(INVALID, f=capi.Frame())
    refused(INVALID, po=o.data_ptr() + 2)
    refused(INVALID, pd=d.data_ptr() + 1)
    over = capi.Frame(); over.depth = o.data_ptr() + 64
    refused(INVALID, f=over)
    over = capi.Frame(); over.color8 = d.data_ptr() + 12 * n - 4
    refused(INVALID, f=over)
    for plane in ("steps_primary", "steps_total", "rays_total", "color8_strips"):
        refused(UNSUPPORTED, f=gb.to_c(only=rr.ALL_PLANES + (plane,)))
    for flags in (1, 4, 16, 32, 1 << 31):
        refused(UNSUPPORTED, s=_settings(vrt, flags=flags))
    for trav in (capi.TRAVERSAL_DENSE, capi.TRAVERSAL_DF, capi.TRAVERSAL_DFJ, 99):
        refused(UNSUPPORTED, s=_settings(vrt, traversal=trav))
    # ... and the context still renders
    assert call() == 0
    engine.synchronize()
    assert not compare_planes(gb.numpy(), exp, rr.ALL_PLANES)
