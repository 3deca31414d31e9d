"""Temporal reprojection for ray cameras on the GPU: k_reproject_cam through the C-ABI against the numpy definition
(tests/reproject_cam_reference.py) bit for bit on the GPU's own planes (vrt_camera_rays -> vrt_render_rays), the identity with
vrt_reproject for the 90-degree pinhole, the optional outputs and the reset, the renderer's frame graph against the Python stages
run by hand, and the C++ mirror against the Python stages."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import raygen_reference as rays
import reproject_cam_common as cc
import reproject_cam_reference as ref
import reproject_common as rc
from test_gpu_cpp_host import APP, _write_dense

pytestmark = pytest.mark.gpu


def _settings(vrt, W, H, ao=2):
    st = vrt.VoxelRenderSettings(targetResolution=(W, H))
    st.fsrSetttings.enable = False
    st.occlusionSettings.numSamples = ao
    return st


def _scene(vrt, engine, seed=1):
    vol, pal, sky, noise = rc.scene_of(vrt, seed)
    return vrt.VoxelScene.from_dense(engine, vol, pal, sky=sky, noise=noise)


def _rays(vrt, engine, cam, W, H):
    """vrt_camera_rays of a vrt_ray_camera block: (origins, dirs) device tensors."""
    import torch
    o = torch.empty((W * H, 3), dtype=torch.float32, device=engine.torch_device)
    d = torch.empty_like(o)
    vrt._capi.check(vrt.lib().vrt_camera_rays(engine.ctx, C.byref(cam), W, H, C.c_void_p(o.data_ptr()), C.c_void_p(d.data_ptr())))
    return o, d


class Gpu:
    """vrt_reproject_camera (or, with push blocks, vrt_reproject) over torch planes with two histories written in turn."""

    def __init__(self, vrt, engine, W, H):
        import torch
        self.vrt, self.engine, self.W, self.H = vrt, engine, W, H
        dev = engine.torch_device
        # filled with a pattern, not zeros: whatever a frame does not write would show
        self.hist = [(torch.full((H, W, 4), 0x5A5A, dtype=torch.int16, device=dev), torch.full((H, W, 4), 0x5A5A5A5A, dtype=torch.int32, device=dev))
                     for _ in range(2)]
        self.resolved = torch.full((H, W, 4), 0x5A, dtype=torch.uint8, device=dev)
        self.motion = torch.full((H, W, 2), 123.0, dtype=torch.float32, device=dev)
        self.cur = -1

    def step(self, cur, prev, color, position, normal, max_history=32, resolved=True, motion=True, reset=False):
        cap, lib = self.vrt._capi, self.vrt.lib()
        if reset:
            self.cur = -1
        nxt = 1 - self.cur if self.cur >= 0 else 0
        hin = cap.History(self.hist[self.cur][0].data_ptr(), self.hist[self.cur][1].data_ptr()) if self.cur >= 0 else None
        hout = cap.History(self.hist[nxt][0].data_ptr(), self.hist[nxt][1].data_ptr())
        args = (color.data_ptr(), position.data_ptr(), normal.data_ptr(), C.byref(hin) if hin is not None else None, C.byref(hout),
                self.resolved.data_ptr() if resolved else None, self.motion.data_ptr() if motion else None)
        if isinstance(cur, cap.RayCamera):
            st = cap.ReprojectSettings()
            lib.vrt_reproject_camera_settings_default(C.byref(cur), self.W, C.byref(st))
            st.max_history = max_history
            cap.check(lib.vrt_reproject_camera(self.engine.ctx, self.W, self.H, C.byref(cur), C.byref(prev), C.byref(st), *args))
        else:
            st = self.vrt.ReprojectSettings(maxHistory=max_history).to_c(cur)
            cap.check(lib.vrt_reproject(self.engine.ctx, self.W, self.H, C.byref(cur), C.byref(prev), C.byref(st), *args))
        self.cur = nxt
        self.engine.synchronize()
        return {"color16": self.hist[nxt][0].cpu().numpy().view(np.uint16), "surface": self.hist[nxt][1].cpu().numpy().view(np.uint32),
                "resolved8": self.resolved.cpu().numpy(), "motion": self.motion.cpu().numpy()}


def _sequence(vrt, oracle, model, W, H):
    """(seed, cameras): the CPU side's choice (tests/test_reproject_cam_cpu.py) -- at 256 pixels and more the first seed whose
    sequence holds every class by the definition's output on the oracle's frames."""
    if W * H >= 256:
        seed, _, cams, _ = cc.pick_scene_seed(vrt, oracle, model, W, H)
        return seed, cams
    return 1, cc.cameras_of(vrt, oracle, model, W, H, rc.scene_of(vrt, 1)[0])


@pytest.mark.parametrize("max_history", (1, 255))
@pytest.mark.parametrize("W,H", cc.SIZES)
@pytest.mark.parametrize("model", cc.MODELS)
def test_kernel_matches_definition(vrt, oracle, engine, model, W, H, max_history):
    """Six frames of the model's moving sequence drawn by the GPU itself (vrt_camera_rays -> vrt_render_rays): every output plane
    of vrt_reproject_camera equals the numpy definition on the same planes, bit for bit, the history out of frame k feeding frame
    k + 1 on both sides; every buffer is filled with a pattern beforehand.  At 256 pixels and more the sequence holds every class
    the model can produce at >= 5 % of the pixels that had a history."""
    seed, cams = _sequence(vrt, oracle, model, W, H)
    sc = _scene(vrt, engine, seed)
    geo = vrt.GeometryStage(engine, _settings(vrt, W, H), sc)
    g = Gpu(vrt, engine, W, H)
    hist, used, results = None, 0, []
    for k, cam in enumerate(cams):
        o, d = _rays(vrt, engine, cam, W, H)
        gb = geo.record_rays(o, d, (W, H), k + 1)
        prev = cams[k - 1] if k else cams[0]
        got = g.step(cam, prev, gb.color, gb.position, gb.normal, max_history)
        pl = gb.numpy()
        exp = ref.reproject(W, H, cam, prev, pl["color8"], pl["position"], pl["normal8"], hist, max_history)
        assert ref.same(got, exp) == [], (k, ref.same(got, exp))
        hist = (exp["color16"], exp["surface"])
        used += int(((exp["surface"][..., 3] >> 24) > 1).sum())
        results.append(exp)
    if W * H >= 256:
        sh = cc.class_shares(results)
        print(f"\n{model} {W}x{H}: scene seed {seed}, shares " + ", ".join(f"{k} {v:.3f}" for k, v in sh.items()))
        assert min(sh[k] for k in cc.NEEDED[model]) >= 0.05, sh
        assert used > 0 or max_history == 1


def test_pinhole_identity(vrt, oracle, engine):
    """Perspective with tan_half == 1.0f: every plane of vrt_reproject_camera equals vrt_reproject's on the same frames -- the
    jittered push blocks of tests/reproject_common.py, drawn by the geometry stage -- in every frame."""
    W, H = 67, 45
    sc = _scene(vrt, engine)
    geo = vrt.GeometryStage(engine, _settings(vrt, W, H), sc)
    pushes = rc.pushes_of(vrt, oracle, W, H)
    cams = []
    for p in pushes:
        c = vrt._capi.RayCamera(); c.model = rays.PERSPECTIVE; c.basis = vrt._capi.Push.from_buffer_copy(p); c.tan_half = 1.0
        cams.append(c)
    a, b = Gpu(vrt, engine, W, H), Gpu(vrt, engine, W, H)
    for k, push in enumerate(pushes):
        gb = geo.record(push)
        want = a.step(push, pushes[max(k - 1, 0)], gb.color, gb.position, gb.normal)
        got = b.step(cams[k], cams[max(k - 1, 0)], gb.color, gb.position, gb.normal)
        assert ref.same(got, want) == [], (k, ref.same(got, want))
    assert ((want["surface"][..., 3] >> 24) > 2).any() and np.abs(want["motion"]).max() > 1.0


def test_panorama_tap_wraps_in_x(vrt, engine):
    """The wrap on the device: a point just past the seam takes its history from column W - 1 (tests/test_reproject_cam_cpu.py has
    the same case for the header)."""
    import torch
    W, H = 8, 4
    at = (3.0, 4.0, 5.0)
    cam = vrt.RayCamera.panorama(at).to_c((W, H))
    P = np.array(at, np.float32) + np.array([-4.0, 0.0, -0.01], np.float32)
    pos = np.zeros((H, W, 4), np.float32); nrm = np.zeros((H, W, 4), np.int8); col = np.zeros((H, W, 4), np.uint8)
    pos[1, 6, :3] = P; nrm[1, 6, :3] = (127, 0, 0); col[1, 6] = (200, 100, 50, 0)
    color16 = np.zeros((H, W, 4), np.uint16); surface = np.zeros((H, W, 4), np.uint32)
    surface[..., :3] = P.view(np.uint32)
    surface[..., 3] = 0x00007F | (5 << 24)
    surface[:, 0, 3] = 0x007F00 | (5 << 24)
    color16[:, W - 1] = 90 << 8
    color16[:, 0] = 250 << 8
    exp = ref.reproject(W, H, cam, cam, col, pos, nrm, (color16, surface))
    assert exp["wrapped"][1, 6] and exp["surface"][1, 6, 3] >> 24 == 6
    g = Gpu(vrt, engine, W, H)
    dev = engine.torch_device
    g.hist[0] = (torch.from_numpy(color16.view(np.int16)).to(dev), torch.from_numpy(surface.view(np.int32)).to(dev))
    g.cur = 0
    got = g.step(cam, cam, torch.from_numpy(col).to(dev), torch.from_numpy(pos).to(dev), torch.from_numpy(nrm).to(dev))
    assert ref.same(got, exp) == []
    assert got["color16"][1, 6, 0] == ((90 << 8) * 5 + (200 << 8) + 3) // 6


def test_optional_outputs_and_reset(vrt, oracle, engine):
    """With a NULL resolved8 or motion the other outputs are what they are with both, and the plane left out is not touched; a
    reset (NULL history in) equals the first frame of a fresh sequence."""
    W, H = 67, 45
    model = "orthographic"
    seed, cams = _sequence(vrt, oracle, model, W, H)
    sc = _scene(vrt, engine, seed)
    geo = vrt.GeometryStage(engine, _settings(vrt, W, H), sc)
    cams = cams[:3]
    planes = []
    for k, cam in enumerate(cams):
        o, d = _rays(vrt, engine, cam, W, H)
        gb = geo.record_rays(o, d, (W, H), k + 1)
        planes.append((gb.color.clone(), gb.position.clone(), gb.normal.clone()))
    full = Gpu(vrt, engine, W, H)
    want = [full.step(cams[k], cams[max(k - 1, 0)], *planes[k]) for k in range(3)]
    for kw in (dict(resolved=False), dict(motion=False), dict(resolved=False, motion=False)):
        g = Gpu(vrt, engine, W, H)
        for k in range(3):
            got = g.step(cams[k], cams[max(k - 1, 0)], *planes[k], **kw)
        names = ["color16", "surface"] + (["resolved8"] if kw.get("resolved", True) else []) + (["motion"] if kw.get("motion", True) else [])
        assert ref.same(got, want[2], names) == [], kw
        if not kw.get("resolved", True):
            assert (got["resolved8"] == 0x5A).all()
        if not kw.get("motion", True):
            assert (got["motion"] == 123.0).all()
    got = full.step(cams[2], cams[1], *planes[2], reset=True)
    pl = [t.cpu().numpy() for t in planes[2]]
    exp = ref.reproject(W, H, cams[2], cams[1], pl[0], pl[1], pl[2], None)
    assert ref.same(got, exp) == [] and ((got["surface"][..., 3] >> 24) == 1).all() and (got["resolved8"] == pl[0]).all()
    fresh = Gpu(vrt, engine, W, H).step(cams[2], cams[1], *planes[2])
    assert ref.same(got, fresh) == []


@pytest.mark.parametrize("model", ("orthographic", "panorama"))
def test_frame_graph_vs_python_stages(vrt, oracle, engine, model):
    """VoxelRenderer(camera=RayCamera..., temporal=True, reproject=True) over 4 moving frames equals the Python stages run by hand
    -- rays -> record_rays -> denoise -> the numpy definition -> blit -- and gBuffer.motion holds the definition's vectors."""
    target = (160, 96)
    vol, pal, sky, noise = rc.scene_of(vrt, 1)
    sc = vrt.VoxelScene.from_dense(engine, vol, pal, sky=sky, noise=noise)
    st = vrt.VoxelRenderSettings(targetResolution=target)
    st.fsrSetttings.scaling = vrt.FsrScaling.QUALITY                     # render at 106 x 64
    st.occlusionSettings.numSamples = 2
    res = st.renderResolution()
    RW, RH = res
    ctrl = vrt.CameraController(position=(12.3, 20.2, -6.0), yaw=90.0, pitch=0.0)
    cam = vrt.RayCamera.orthographic(ctrl, 14.0) if model == "orthographic" else vrt.RayCamera.panorama(tuple(ctrl.position))
    r = vrt.VoxelRenderer(engine, st, sc, camera=cam, temporal=True, reproject=True)
    geo, den = vrt.GeometryStage(engine, st, sc), vrt.DenoiserStage(engine, st)
    hist, prev, moved = None, None, 0.0
    for f in range(4):
        if model == "orthographic":
            ctrl.mouse(2.0, 0.0)
            ctrl.update(1.0 / 60.0, 0.1, 0.5)
        else:
            cam.camera = vrt.CameraController(position=(12.3 + 0.4 * f, 20.2 + 0.2 * f, -6.0 + 0.3 * f))      # in front of the volume
        r.update(1.0 / 60.0)
        img = r.render()
        engine.synchronize()
        cur = cam.to_c(res, r.jitter)
        o, d = cam.rays(engine, res, r.jitter)
        gb = geo.record_rays(o, d, res, r.frameCount)
        dimg = den.record(gb.color, gb.normal, gb.position)
        engine.synchronize()
        pl = gb.numpy()
        exp = ref.reproject(RW, RH, cur, prev if prev is not None else cur, dimg.cpu().numpy(), pl["position"], pl["normal8"], hist)
        hist, prev = (exp["color16"], exp["surface"]), cur
        got = img.cpu().numpy()
        assert got.shape == (target[1], target[0], 4)
        assert (got == oracle.blit(exp["resolved8"], target[0], target[1])).all(), f
        assert (r.gBuffer.motion.cpu().numpy().view(np.uint32) == exp["motion"].view(np.uint32)).all(), f
        h16, hs = r.upscaler.history()
        assert (h16 == exp["color16"]).all() and (hs == exp["surface"]).all()
        moved = max(moved, float(np.abs(exp["motion"]).max()))
    assert moved > 0.5 and ((exp["surface"][..., 3] >> 24) == 4).any()


def test_cpp_app_projection_reproject_matches_python(vrt, oracle, engine, tmp_path):
    """vrt_app --projection ortho:20 --temporal --reproject --fly ... --frames 4: the C++ mirror's image equals, byte for byte, the
    Python stages run over the four push blocks the app itself dumped."""
    assert os.path.exists(APP), "build with __graft_entry__.build()"
    vol, pal, sky, noise = rc.scene_of(vrt, 1)
    dense = tmp_path / "scene.vrtd"
    _write_dense(dense, vol, pal, sky, noise)
    raw, pushf = tmp_path / "out.rgba", tmp_path / "pushes.bin"
    r = subprocess.run([APP, "--dense", str(dense), "--width", "160", "--height", "96", "--pos", "12.3", "20.2", "-6", "--ao", "2",
                        "--projection", "ortho:20", "--temporal", "--reproject", "--fly", "0.1", "0.5", "2.0", "--frames", "4",
                        "--raw", str(raw), "--dump-pushes", str(pushf)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    blob = pushf.read_bytes()
    assert len(blob) == 4 * 96
    pushes = [vrt._capi.Push.from_buffer_copy(blob[96 * k: 96 * k + 96]) for k in range(4)]
    assert [p.frame for p in pushes] == [1, 2, 3, 4] and pushes[0].cam_pos[0] != pushes[3].cam_pos[0]
    st = vrt.VoxelRenderSettings(targetResolution=(160, 96))
    st.occlusionSettings.numSamples = 2
    res = st.renderResolution()
    assert tuple(pushes[0].screen_size) == res == (94, 56)
    sc = vrt.VoxelScene.from_dense(engine, vol, pal, sky=sky, noise=noise)
    geo, den, up = vrt.GeometryStage(engine, st, sc), vrt.DenoiserStage(engine, st), vrt.UpscalerStage(engine, st)
    for p in pushes:
        cam = vrt._capi.RayCamera(); cam.model = rays.ORTHOGRAPHIC; cam.basis = vrt._capi.Push.from_buffer_copy(p)
        cam.tan_half, cam.half_width = 1.0, 20.0
        o, d = _rays(vrt, engine, cam, res[0], res[1])
        gb = geo.record_rays(o, d, res, p.frame)
        img = up.record_reprojected_camera(den.record(gb.color, gb.normal, gb.position), gb, cam)
    engine.synchronize()
    got = np.frombuffer(raw.read_bytes(), np.uint8).reshape(96, 160, 4)
    assert (got == img.cpu().numpy()).all(), int((got != img.cpu().numpy()).sum())
    assert ((up.history()[1][..., 3] >> 24) == 4).any()                   # history survived the motion
    # the accumulation stays refused for a projection
    r = subprocess.run([APP, "--dense", str(dense), "--width", "160", "--height", "96", "--projection", "ortho:20", "--temporal",
                        "--raw", str(raw)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "--projection" in r.stderr
