"""Temporal upsampling for ray cameras on the GPU: k_upsample_cam<0..2> through the C-ABI against the numpy definition
(tests/upsample_cam_reference.py) bit for bit on the GPU's own planes (vrt_camera_rays_offset -> vrt_render_rays),
k_camera_rays_offset against its definition, the identity with vrt_upsample for the 90-degree pinhole, the renderer's frame graph
against the stages run by hand, and both new entry points on the three kinds of stream behind a busy device."""
import ctypes as C

import numpy as np
import pytest

import reproject_common as rc
import stream_common as sc
import upsample_cam_common as uc
import upsample_cam_reference as ref
from test_raygen_offset_cpu import OFFSETS, SIZES, _cam

pytestmark = pytest.mark.gpu


def _settings(vrt, w, h, ao=2):
    st = vrt.VoxelRenderSettings(targetResolution=(w, h))
    st.fsrSetttings.enable = False
    st.occlusionSettings.numSamples = ao
    return st


def _scene(vrt, engine, model):
    _, pal, sky, noise = rc.scene_of(vrt, 1)
    return vrt.VoxelScene.from_dense(engine, uc.volume_of(vrt, model), pal, sky=sky, noise=noise)


def _rays(vrt, engine, cam, W, H, offset=None):
    """vrt_camera_rays_offset (offset None: vrt_camera_rays) of a vrt_ray_camera block: (origins, dirs) device tensors."""
    import torch
    o = torch.full((W * H, 3), 7.0, dtype=torch.float32, device=engine.torch_device)
    d = torch.full((W * H, 3), 7.0, dtype=torch.float32, device=engine.torch_device)
    if offset is None:
        vrt._capi.check(vrt.lib().vrt_camera_rays(engine.ctx, C.byref(cam), W, H, C.c_void_p(o.data_ptr()), C.c_void_p(d.data_ptr())))
    else:
        off = (C.c_float * 2)(*offset)
        vrt._capi.check(vrt.lib().vrt_camera_rays_offset(engine.ctx, C.byref(cam), W, H, off, C.c_void_p(o.data_ptr()), C.c_void_p(d.data_ptr())))
    return o, d


class Gpu:
    """vrt_upsample_camera (or, with push blocks, vrt_upsample) over torch planes with two histories written in turn."""

    def __init__(self, vrt, engine, size):
        import torch
        self.vrt, self.engine, self.size = vrt, engine, size
        w, h, TW, TH = size
        dev = engine.torch_device
        # filled with a pattern, not zeros: whatever a frame does not write would show
        self.hist = [(torch.full((TH, TW, 4), 0x5A5A, dtype=torch.int16, device=dev), torch.full((TH, TW, 4), 0x5A5A5A5A, dtype=torch.int32, device=dev))
                     for _ in range(2)]
        self.resolved = torch.full((TH, TW, 4), 0x5A, dtype=torch.uint8, device=dev)
        self.motion = torch.full((TH, TW, 2), 123.0, dtype=torch.float32, device=dev)
        self.cur = -1

    def enqueue(self, cur, prev, color, position, normal, resolved=True, motion=True):
        cap, lib = self.vrt._capi, self.vrt.lib()
        w, h, TW, TH = self.size
        nxt = 1 - self.cur if self.cur >= 0 else 0
        hin = cap.History(self.hist[self.cur][0].data_ptr(), self.hist[self.cur][1].data_ptr()) if self.cur >= 0 else None
        hout = cap.History(self.hist[nxt][0].data_ptr(), self.hist[nxt][1].data_ptr())
        args = (color.data_ptr(), position.data_ptr(), normal.data_ptr(), C.byref(hin) if hin is not None else None, C.byref(hout),
                self.resolved.data_ptr() if resolved else None, self.motion.data_ptr() if motion else None)
        if isinstance(cur, cap.RayCamera):
            cap.check(lib.vrt_upsample_camera(self.engine.ctx, w, h, TW, TH, C.byref(cur), C.byref(prev), None, *args))
        else:
            cap.check(lib.vrt_upsample(self.engine.ctx, w, h, TW, TH, C.byref(cur), C.byref(prev), None, *args))
        self.cur = nxt

    def read(self):
        return {"color16": self.hist[self.cur][0].cpu().numpy().view(np.uint16), "surface": self.hist[self.cur][1].cpu().numpy().view(np.uint32),
                "resolved8": self.resolved.cpu().numpy(), "motion": self.motion.cpu().numpy()}

    def step(self, *a, **kw):
        self.enqueue(*a, **kw)
        self.engine.synchronize()
        return self.read()


CASES = [(m, s, {}) for m in uc.MODELS for s in uc.SIZES] + [("panorama", uc.SEAM, dict(moving=False, frames=4, offset_list=uc.SEAM_OFFSETS)),
                                                               ("panorama", uc.SEAM, dict(slide=0.45))]


@pytest.mark.parametrize("planes", ("all", "none"))
@pytest.mark.parametrize("model,size,kw", CASES, ids=["%s-%dx%d-%dx%d%s" % ((m,) + s + ("-" + "-".join(k) if k else "",)) for m, s, k in CASES])
def test_kernel_matches_definition(vrt, oracle, engine, model, size, kw, planes):
    """The CPU tests' sequences drawn by the GPU itself (vrt_camera_rays_offset -> vrt_render_rays): every output plane of
    vrt_upsample_camera equals the numpy definition on the same planes, bit for bit, the history out of frame k feeding frame
    k + 1 on both sides; with resolved8 and motion NULL the histories are the same and the two planes keep their pattern."""
    w, h, TW, TH = size
    cams, raycams, offs = uc.sequence(vrt, oracle, model, w, h, TW, **kw)
    geo = vrt.GeometryStage(engine, _settings(vrt, w, h), _scene(vrt, engine, model))
    g = Gpu(vrt, engine, size)
    hist, used, wrapped, seam = None, 0, 0, 0
    for k, cam in enumerate(cams):
        o, d = _rays(vrt, engine, raycams[k], w, h, offs[k])
        gb = geo.record_rays(o, d, (w, h), k + 1)
        prev = cams[k - 1] if k else cams[0]
        got = g.step(cam, prev, gb.color, gb.position, gb.normal, resolved=planes == "all", motion=planes == "all")
        pl = gb.numpy()
        exp = ref.upsample(w, h, TW, TH, cam, prev, pl["color8"], pl["position"], pl["normal8"], hist)
        names = ("color16", "surface", "resolved8", "motion") if planes == "all" else ("color16", "surface")
        assert ref.same(got, exp, names) == [], (k, ref.same(got, exp, names))
        if planes == "none":
            assert (got["resolved8"] == 0x5A).all() and (got["motion"] == 123.0).all()
        hist = (exp["color16"], exp["surface"])
        used += int(((exp["surface"][..., 3] >> 24) > 1).sum())
        wrapped += int(exp["wrapped"].sum()); seam += int(exp["seam_alpha"].sum())
    if w * h >= 256:
        assert used > 0
    if "slide" in kw:
        assert wrapped > 0
    if "offset_list" in kw:
        assert seam > 0


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("model", (ref.PERSPECTIVE, ref.ORTHOGRAPHIC, ref.PANORAMA))
def test_rays_offset_match_definition(vrt, engine, model, W, H, offset):
    cam = _cam(vrt, model, (W, H), jitter=(0.3, -0.2))
    o, d = _rays(vrt, engine, cam, W, H, offset)
    engine.synchronize()
    eo, ed = ref.camera_rays_offset(cam, W, H, offset)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    assert (bits(o.cpu().numpy()) == bits(eo)).all() and (bits(d.cpu().numpy()) == bits(ed)).all()
    if offset == (0.0, 0.0):
        zo, zd = _rays(vrt, engine, cam, W, H)
        engine.synchronize()
        assert (bits(o.cpu().numpy()) == bits(zo.cpu().numpy())).all() and (bits(d.cpu().numpy()) == bits(zd.cpu().numpy())).all()


def test_pinhole_identity(vrt, oracle, engine):
    """Perspective with tan_half == 1.0f: every plane of vrt_upsample_camera equals vrt_upsample's on the same frames -- jittered push
    blocks drawn by the geometry stage -- in every frame."""
    size = (37, 21, 64, 36)
    w, h = size[:2]
    _, pal, sky, noise = rc.scene_of(vrt, 1)
    geo = vrt.GeometryStage(engine, _settings(vrt, w, h), _scene(vrt, engine, "perspective"))
    pushes = rc.pushes_of(vrt, oracle, w, h, uc.FRAMES)
    cams = []
    for p in pushes:
        c = vrt._capi.RayCamera(); c.model = ref.PERSPECTIVE; c.basis = vrt._capi.Push.from_buffer_copy(p); c.tan_half = 1.0
        c.basis.camera_jitter[:] = [0.0, 0.0]
        cams.append(c)
    a, b = Gpu(vrt, engine, size), Gpu(vrt, engine, size)
    for k, push in enumerate(pushes):
        gb = geo.record(push)
        want = a.step(push, pushes[max(k - 1, 0)], gb.color, gb.position, gb.normal)
        got = b.step(cams[k], cams[max(k - 1, 0)], gb.color, gb.position, gb.normal)
        assert ref.same(got, want) == [], (k, ref.same(got, want))
    assert ((want["surface"][..., 3] >> 24) > 2).any() and np.abs(want["motion"]).max() > 1.0


@pytest.mark.parametrize("model", uc.MODELS)
def test_frame_graph_vs_stages(vrt, oracle, engine, model):
    """VoxelRenderer(camera=RayCamera..., temporal=True, reproject=True, upsample=True) over 4 moving frames at 24x14 -> 48x28 equals
    the stages run by hand -- rays (offset or jittered) -> record_rays -> denoise -> the numpy definition -- in the image, the
    history and the display-resolution motion.  (The parent refuses the combination with a ValueError.)"""
    target = (48, 28)
    st = vrt.VoxelRenderSettings(targetResolution=target)
    st.fsrSetttings.scaling = vrt.FsrScaling.PERFORMANCE                 # render at 24 x 14
    st.occlusionSettings.numSamples = 2
    res = st.renderResolution()
    assert tuple(res) == (24, 14)
    sc_ = _scene(vrt, engine, model)
    at = uc.ROOM_AT if model == "panorama" else (12.3, 20.2, -6.0)
    ctrl = vrt.CameraController(position=at, yaw=90.0, pitch=0.0)
    cam = {"perspective": lambda: vrt.RayCamera.perspective(ctrl, uc.FOV_DEG), "orthographic": lambda: vrt.RayCamera.orthographic(ctrl, uc.HALF_WIDTH),
           "panorama": lambda: vrt.RayCamera.panorama(at)}[model]()
    r = vrt.VoxelRenderer(engine, st, sc_, camera=cam, temporal=True, reproject=True, upsample=True)
    geo, den = vrt.GeometryStage(engine, st, sc_), vrt.DenoiserStage(engine, st)
    hist, prev, moved, offsets = None, None, 0.0, 0
    for f in range(4):
        if model == "panorama":
            cam.camera = vrt.CameraController(position=(at[0] + 0.4 * f, at[1] - 0.2 * f, at[2] + 0.3 * f))
        else:
            ctrl.mouse(2.0, 0.0)
            ctrl.update(1.0 / 60.0, 0.1, 0.5)
        r.update(1.0 / 60.0)
        img = r.render()
        engine.synchronize()
        cur = cam.to_c(res)
        if model == "perspective":
            o, d = cam.rays(engine, res, r.jitter)
        else:
            o, d = cam.rays(engine, res, offset=r.jitter)
            offsets += r.jitter != (0.0, 0.0)
        gb = geo.record_rays(o, d, res, r.frameCount)
        dimg = den.record(gb.color, gb.normal, gb.position)
        engine.synchronize()
        pl = gb.numpy()
        exp = ref.upsample(res[0], res[1], target[0], target[1], cur, prev if prev is not None else cur, dimg.cpu().numpy(), pl["position"],
                           pl["normal8"], hist)
        hist, prev = (exp["color16"], exp["surface"]), cur
        got = img.cpu().numpy()
        assert got.shape == (target[1], target[0], 4) and (got == exp["resolved8"]).all(), f
        assert (r.upscaler.motion.cpu().numpy().view(np.uint32) == exp["motion"].view(np.uint32)).all(), f
        h16, hs = r.upscaler.history()
        assert (h16 == exp["color16"]).all() and (hs == exp["surface"]).all()
        moved = max(moved, float(np.abs(exp["motion"]).max()))
    assert moved > 0.25 and ((exp["surface"][..., 3] >> 24) > 1).any() and (model == "perspective" or offsets >= 3)


def test_cpp_app_projection_upsample_matches_python(vrt, oracle, engine, tmp_path):
    """vrt_app --projection ortho:20 --temporal --reproject --upsample --fly ... --frames 4: the C++ mirror's image equals, byte for
    byte, the Python stages run over the four push blocks the app itself dumped -- their camera_jitter as the rays' offset, the
    pass camera without it."""
    import os
    import subprocess
    from test_gpu_cpp_host import APP, _write_dense
    assert os.path.exists(APP), "build with __graft_entry__.build()"
    vol, pal, sky, noise = rc.scene_of(vrt, 1)
    dense = tmp_path / "scene.vrtd"
    _write_dense(dense, vol, pal, sky, noise)
    raw, pushf = tmp_path / "out.rgba", tmp_path / "pushes.bin"
    r = subprocess.run([APP, "--dense", str(dense), "--width", "160", "--height", "96", "--pos", "12.3", "20.2", "-6", "--ao", "2",
                        "--projection", "ortho:20", "--temporal", "--reproject", "--upsample", "--fly", "0.1", "0.5", "2.0", "--frames", "4",
                        "--raw", str(raw), "--dump-pushes", str(pushf)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    blob = pushf.read_bytes()
    assert len(blob) == 4 * 96
    pushes = [vrt._capi.Push.from_buffer_copy(blob[96 * k: 96 * k + 96]) for k in range(4)]
    assert [p.frame for p in pushes] == [1, 2, 3, 4] and any(p.camera_jitter[0] != 0 for p in pushes)
    st = vrt.VoxelRenderSettings(targetResolution=(160, 96))
    st.occlusionSettings.numSamples = 2
    res = st.renderResolution()
    assert tuple(pushes[0].screen_size) == tuple(res)
    sc_ = vrt.VoxelScene.from_dense(engine, vol, pal, sky=sky, noise=noise)
    geo, den, up = vrt.GeometryStage(engine, st, sc_), vrt.DenoiserStage(engine, st), vrt.UpscalerStage(engine, st)
    for p in pushes:
        cam = vrt._capi.RayCamera(); cam.model = ref.ORTHOGRAPHIC; cam.basis = vrt._capi.Push.from_buffer_copy(p)
        cam.tan_half, cam.half_width = 1.0, 20.0
        off = tuple(p.camera_jitter)
        cam.basis.camera_jitter[:] = [0.0, 0.0]
        o, d = _rays(vrt, engine, cam, res[0], res[1], off if off != (0.0, 0.0) else None)
        gb = geo.record_rays(o, d, res, p.frame)
        img = up.record_upsampled_camera(den.record(gb.color, gb.normal, gb.position), gb, cam)
    engine.synchronize()
    got = np.frombuffer(raw.read_bytes(), np.uint8).reshape(96, 160, 4)
    assert (got == img.cpu().numpy()).all(), int((got != img.cpu().numpy()).sum())
    assert ((up.history()[1][..., 3] >> 24) == 4).any()                   # history survived the motion


@pytest.mark.parametrize("kind", sc.KINDS)
def test_streams_behind_a_busy_device(vrt, oracle, kind):
    """Both new entry points on the HIP null stream, the context's own stream and a side stream of the caller: a stall of
    tests/stream_common.py's size is enqueued, then -- with no synchronise by the caller -- two frames of vrt_camera_rays_offset
    and vrt_upsample_camera that hand their history pair on; one vrt_ctx_synchronize, then every output against the definitions,
    bit for bit.  Run once."""
    import torch
    size = (24, 14, 48, 28)
    w, h, TW, TH = size
    model = "panorama"                                                   # the model with tables to upload on the stream
    cams, raycams, offs, frames, exp = uc.case(vrt, oracle, model, size)
    side = torch.cuda.Stream() if kind == "side" else None
    with torch.cuda.stream(side if side is not None else torch.cuda.default_stream()):
        engine = vrt.Engine(0, use_torch_stream=kind != "own")
        dev = engine.torch_device
        lib, cap = vrt.lib(), vrt._capi
        g = Gpu(vrt, engine, size)
        up = [[torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in frames[k]] for k in range(2)]
        ray_out = [(torch.full((w * h, 3), 7.0, dtype=torch.float32, device=dev), torch.full((w * h, 3), 7.0, dtype=torch.float32, device=dev))
                   for _ in range(2)]
        res = [torch.full((TH, TW, 4), 0x5A, dtype=torch.uint8, device=dev) for _ in range(2)]
        stall_t, stall_p = None, C.c_void_p()
        if kind == "own":
            cap.check(lib.vrt_device_alloc(engine.ctx, sc.STALL_BYTES, C.byref(stall_p)))
        else:
            stall_t = torch.zeros(sc.STALL_BYTES // 4, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        for k in range(sc.STALL_PASSES):                                 # the stall
            if kind == "own":
                cap.check(lib.vrt_memset(engine.ctx, stall_p, k, sc.STALL_BYTES))
            else:
                stall_t.add_(1.0)
        for k in range(2):                                               # the sequence: no synchronise in between
            off = (C.c_float * 2)(*offs[k])
            cap.check(lib.vrt_camera_rays_offset(engine.ctx, C.byref(raycams[k]), w, h, off, C.c_void_p(ray_out[k][0].data_ptr()),
                                                 C.c_void_p(ray_out[k][1].data_ptr())))
            g.resolved = res[k]
            g.enqueue(cams[k], cams[max(k - 1, 0)], *up[k])
        engine.synchronize()                                             # once
        if kind == "own":
            torch.cuda.synchronize()
        bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
        for k in range(2):
            eo, ed = ref.camera_rays_offset(raycams[k], w, h, offs[k])
            assert (bits(ray_out[k][0].cpu().numpy()) == bits(eo)).all() and (bits(ray_out[k][1].cpu().numpy()) == bits(ed)).all(), (kind, k)
            assert (res[k].cpu().numpy() == exp[k]["resolved8"]).all(), (kind, k)
        assert ref.same(g.read(), exp[1]) == [], kind
        if kind == "own":
            lib.vrt_device_free(engine.ctx, stall_p)
