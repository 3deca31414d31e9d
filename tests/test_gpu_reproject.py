"""Temporal reprojection on the GPU: k_reproject through the C-ABI against the numpy definition (tests/reproject_reference.py) bit
for bit on the GPU's own rendered planes, the optional outputs and the reset, the renderer's frame graph against the oracle
chain, and the C++ mirror against the Python stages."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import reproject_common as rc
import reproject_reference as ref
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


class Gpu:
    """vrt_reproject over torch planes with two histories written in turn."""

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
        cap = self.vrt._capi
        if reset:
            self.cur = -1
        nxt = 1 - self.cur if self.cur >= 0 else 0
        hin = cap.History(self.hist[self.cur][0].data_ptr(), self.hist[self.cur][1].data_ptr()) if self.cur >= 0 else None
        hout = cap.History(self.hist[nxt][0].data_ptr(), self.hist[nxt][1].data_ptr())
        st = self.vrt.ReprojectSettings(maxHistory=max_history).to_c(cur)
        cap.check(self.vrt.lib().vrt_reproject(self.engine.ctx, self.W, self.H, C.byref(cur), C.byref(prev), C.byref(st), color.data_ptr(),
                                               position.data_ptr(), normal.data_ptr(), C.byref(hin) if hin is not None else None, C.byref(hout),
                                               self.resolved.data_ptr() if resolved else None, self.motion.data_ptr() if motion else None))
        self.cur = nxt
        self.engine.synchronize()
        return {"color16": self.hist[nxt][0].cpu().numpy().view(np.uint16), "surface": self.hist[nxt][1].cpu().numpy().view(np.uint32),
                "resolved8": self.resolved.cpu().numpy(), "motion": self.motion.cpu().numpy()}


@pytest.mark.parametrize("max_history", (1, 255))
@pytest.mark.parametrize("W,H", rc.SIZES)
def test_kernel_matches_definition(vrt, oracle, engine, W, H, max_history):
    """Six frames of the moving sequence rendered by the GPU itself: every output plane of vrt_reproject equals the numpy
    definition on the same planes, bit for bit, the history out of frame k feeding frame k + 1 on both sides."""
    sc = _scene(vrt, engine)
    geo = vrt.GeometryStage(engine, _settings(vrt, W, H), sc)
    pushes = rc.pushes_of(vrt, oracle, W, H)
    g = Gpu(vrt, engine, W, H)
    hist, used, results = None, 0, []
    for k, push in enumerate(pushes):
        gb = geo.record(push)
        prev = pushes[k - 1] if k else pushes[0]
        got = g.step(push, prev, gb.color, gb.position, gb.normal, max_history)
        pl = gb.numpy()
        exp = ref.reproject(W, H, push, prev, pl["color8"], pl["position"], pl["normal8"], hist, max_history)
        assert ref.same(got, exp) == [], (k, ref.same(got, exp))
        hist = (exp["color16"], exp["surface"])
        used += int(((exp["surface"][..., 3] >> 24) > 1).sum())
        results.append(exp)
    if W * H >= 256:
        # the sequence (all frames that had a history, as on the CPU side) holds every class the kernel has a path for
        sh = rc.class_shares(results)
        assert min(sh[k] for k in rc.NEEDED) >= 0.05, sh
        assert used > 0 or max_history == 1


def test_optional_outputs_and_reset(vrt, oracle, engine):
    """With a NULL resolved8 or motion the other outputs are what they are with both, and the plane left out is not touched; a
    reset (NULL history in) equals the first frame of a fresh sequence."""
    W, H = 67, 45
    sc = _scene(vrt, engine)
    geo = vrt.GeometryStage(engine, _settings(vrt, W, H), sc)
    pushes = rc.pushes_of(vrt, oracle, W, H, frames=3)
    planes = []
    for p in pushes:
        gb = geo.record(p)
        planes.append((gb.color.clone(), gb.position.clone(), gb.normal.clone()))
    full = Gpu(vrt, engine, W, H)
    want = [full.step(pushes[k], pushes[max(k - 1, 0)], *planes[k]) for k in range(3)]
    for kw in (dict(resolved=False), dict(motion=False), dict(resolved=False, motion=False)):
        g = Gpu(vrt, engine, W, H)
        for k in range(3):
            got = g.step(pushes[k], pushes[max(k - 1, 0)], *planes[k], **kw)
        names = ["color16", "surface"] + (["resolved8"] if kw.get("resolved", True) else []) + (["motion"] if kw.get("motion", True) else [])
        assert ref.same(got, want[2], names) == [], kw
        if not kw.get("resolved", True):
            assert (got["resolved8"] == 0x5A).all()
        if not kw.get("motion", True):
            assert (got["motion"] == 123.0).all()
    # reset in mid-sequence: frame 2 without history == frame 2 as the first frame of a new sequence
    got = full.step(pushes[2], pushes[1], *planes[2], reset=True)
    pl = [t.cpu().numpy() for t in planes[2]]
    exp = ref.reproject(W, H, pushes[2], pushes[1], pl[0], pl[1], pl[2], None)
    assert ref.same(got, exp) == [] and ((got["surface"][..., 3] >> 24) == 1).all() and (got["resolved8"] == pl[0]).all()
    fresh = Gpu(vrt, engine, W, H).step(pushes[2], pushes[1], *planes[2])
    assert ref.same(got, fresh) == []


def _fly(r, frames, mouse=2.0, forward=0.1, strafe=0.5):
    """frames of a moving renderer: yields (push, image); update() advances jitter and frame as well."""
    for _ in range(frames):
        r.camera.mouse(mouse, 0.0)
        r.update(1.0 / 60.0, forward, strafe)
        push = r.push_constants()
        yield push, r.render()


def test_frame_graph_vs_oracle_chain(vrt, oracle, engine):
    """VoxelRenderer(temporal=True, reproject=True) over 5 moving, jittered frames equals oracle render -> oracle.denoise -> the
    definition -> oracle.blit, and gBuffer.motion holds the definition's vectors; with reproject=False the image is the
    accumulation path's, as before."""
    target = (160, 96)
    vol, pal, sky, noise = rc.scene_of(vrt, 1)
    sc = vrt.VoxelScene.from_dense(engine, vol, pal, sky=sky, noise=noise)
    st = vrt.VoxelRenderSettings(targetResolution=target)
    st.fsrSetttings.scaling = vrt.FsrScaling.QUALITY                     # render at 106 x 64
    st.occlusionSettings.numSamples = 2
    RW, RH = st.renderResolution()
    osn, pr = oracle.OracleScene(vol, pal, sky=sky, noise=noise), oracle.params_from(st.to_c())
    r = vrt.VoxelRenderer(engine, st, sc, temporal=True, reproject=True)
    r.camera.position = np.array([12.3, 20.2, -6.0], np.float32); r.camera.updateDirectionVectors()
    hist, prev, moved = None, None, 0.0
    for f, (push, img) in enumerate(_fly(r, 5)):
        engine.synchronize()
        fr = oracle.render(osn, push, pr, planes=["color8", "normal8", "position"], nthreads=8)
        den = oracle.denoise(fr["color8"], fr["normal8"], fr["position"])
        exp = ref.reproject(RW, RH, push, prev if prev is not None else push, den, fr["position"], fr["normal8"], hist)
        hist, prev = (exp["color16"], exp["surface"]), push
        got = img.cpu().numpy()
        assert got.shape == (target[1], target[0], 4)
        assert (got == oracle.blit(exp["resolved8"], target[0], target[1])).all(), f
        assert (r.gBuffer.motion.cpu().numpy().view(np.uint32) == exp["motion"].view(np.uint32)).all(), f
        h16, hs = r.upscaler.history()
        assert (h16 == exp["color16"]).all() and (hs == exp["surface"]).all()
        moved = max(moved, float(np.abs(exp["motion"]).max()))
    assert moved > 1.0 and ((exp["surface"][..., 3] >> 24) == 5).any()
    # reset starts a new sequence
    r.upscaler.reset()
    push, img = next(_fly(r, 1))
    engine.synchronize()
    fr = oracle.render(osn, push, pr, planes=["color8", "normal8", "position"], nthreads=8)
    den = oracle.denoise(fr["color8"], fr["normal8"], fr["position"])
    assert (img.cpu().numpy() == oracle.blit(den, target[0], target[1])).all()
    # reproject=False (the default): the accumulation path, untouched -- two frames of a camera at rest against the exact mean
    r0 = vrt.VoxelRenderer(engine, st, sc, temporal=True)
    assert r0.reproject is False
    r0.camera.position = np.array([12.3, 20.2, -6.0], np.float32); r0.camera.updateDirectionVectors()
    acc = np.zeros((RH, RW, 4), np.int64)
    for f in range(2):
        r0.update(0.0)
        img = r0.render().cpu().numpy()
        engine.synchronize()
        fr = oracle.render(osn, r0.push_constants(), pr, planes=["color8", "normal8", "position"], nthreads=8)
        acc += oracle.denoise(fr["color8"], fr["normal8"], fr["position"])
        assert (img == oracle.blit(((2 * acc + (f + 1)) // (2 * (f + 1))).astype(np.uint8), target[0], target[1])).all()
        assert not r0.gBuffer.motion.any()                                # the geometry stage goes on writing 0


def test_cpp_app_reproject_matches_python(vrt, oracle, engine, tmp_path):
    """vrt_app --temporal --reproject --fly ... --frames 4: the C++ mirror's image equals, byte for byte, the Python stages run
    over the four push blocks the app itself computed (its CameraController is C++ libm, as in test_gpu_cpp_host.py)."""
    assert os.path.exists(APP), "build with __graft_entry__.build()"
    vol, pal, sky, noise = rc.scene_of(vrt, 1)
    dense = tmp_path / "scene.vrtd"
    _write_dense(dense, vol, pal, sky, noise)
    raw, pushf = tmp_path / "out.rgba", tmp_path / "pushes.bin"
    r = subprocess.run([APP, "--dense", str(dense), "--width", "160", "--height", "96", "--pos", "12.3", "20.2", "-6", "--ao", "2",
                        "--temporal", "--reproject", "--fly", "0.1", "0.5", "2.0", "--frames", "4", "--raw", str(raw),
                        "--dump-pushes", str(pushf)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    blob = pushf.read_bytes()
    assert len(blob) == 4 * 96
    pushes = [vrt._capi.Push.from_buffer_copy(blob[96 * k: 96 * k + 96]) for k in range(4)]
    assert [p.frame for p in pushes] == [1, 2, 3, 4] and pushes[0].cam_pos[0] != pushes[3].cam_pos[0]
    st = vrt.VoxelRenderSettings(targetResolution=(160, 96))
    st.occlusionSettings.numSamples = 2
    assert tuple(pushes[0].screen_size) == st.renderResolution() == (94, 56)
    sc = vrt.VoxelScene.from_dense(engine, vol, pal, sky=sky, noise=noise)
    geo, den, up = vrt.GeometryStage(engine, st, sc), vrt.DenoiserStage(engine, st), vrt.UpscalerStage(engine, st)
    for p in pushes:
        gb = geo.record(p)
        img = up.record_reprojected(den.record(gb.color, gb.normal, gb.position), gb, p)
    engine.synchronize()
    got = np.frombuffer(raw.read_bytes(), np.uint8).reshape(96, 160, 4)
    assert (got == img.cpu().numpy()).all(), int((got != img.cpu().numpy()).sum())
    assert ((up.history()[1][..., 3] >> 24) == 4).any()                   # history survived the motion
