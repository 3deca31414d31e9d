"""Temporal upsampling on the GPU: k_upsample through the C-ABI against the numpy definition (tests/upsample_reference.py) bit for
bit on oracle-rendered sequences, the optional outputs, the renderer's frame graph, the C++ mirror, and vrt_reproject left as it
was."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import reproject_common as rc
import reproject_reference as rref
import upsample_common as uc
import upsample_reference as ref
from test_gpu_cpp_host import APP, _write_dense

pytestmark = pytest.mark.gpu

_SEQ = {}


def sequence(vrt, oracle, pair):
    """(pushes, frames) of a pair's moving sequence, rendered by the oracle once per session and left unchanged."""
    if pair not in _SEQ:
        pushes = uc.pushes_of(vrt, oracle, pair)
        _SEQ[pair] = (pushes, rc.oracle_frames(vrt, oracle, uc.seed_of(pair), pushes))
    return _SEQ[pair]


class Gpu:
    """vrt_upsample over torch planes with two display-resolution histories written in turn."""

    def __init__(self, vrt, engine, pair):
        import torch
        self.vrt, self.engine, self.pair, self.torch = vrt, engine, pair, torch
        w, h, TW, TH = pair
        dev = engine.torch_device
        a, b = C.c_size_t(), C.c_size_t()
        vrt._capi.check(vrt.lib().vrt_history_bytes(TW, TH, C.byref(a), C.byref(b)))
        assert (a.value, b.value) == (TW * TH * 8, TW * TH * 16)
        # filled with a pattern, not zeros: whatever a frame does not write would show
        self.hist = [(torch.full((a.value // 2,), 0x5A5A, dtype=torch.int16, device=dev).view(TH, TW, 4),
                      torch.full((b.value // 4,), 0x5A5A5A5A, dtype=torch.int32, device=dev).view(TH, TW, 4)) for _ in range(2)]
        self.resolved = torch.full((TH, TW, 4), 0x5A, dtype=torch.uint8, device=dev)
        self.motion = torch.full((TH, TW, 2), 123.0, dtype=torch.float32, device=dev)
        self.cur = -1

    def step(self, cur, prev, frame, max_history=32, resolved=True, motion=True):
        cap, torch, dev = self.vrt._capi, self.torch, self.engine.torch_device
        w, h, TW, TH = self.pair
        color, position, normal = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in frame)
        nxt = 1 - self.cur if self.cur >= 0 else 0
        hin = cap.History(self.hist[self.cur][0].data_ptr(), self.hist[self.cur][1].data_ptr()) if self.cur >= 0 else None
        hout = cap.History(self.hist[nxt][0].data_ptr(), self.hist[nxt][1].data_ptr())
        st = self.vrt.ReprojectSettings(maxHistory=max_history).to_c(cur)
        cap.check(self.vrt.lib().vrt_upsample(self.engine.ctx, w, h, TW, TH, C.byref(cur), C.byref(prev), C.byref(st), color.data_ptr(),
                                              position.data_ptr(), normal.data_ptr(), C.byref(hin) if hin is not None else None, C.byref(hout),
                                              self.resolved.data_ptr() if resolved else None, self.motion.data_ptr() if motion else None))
        self.cur = nxt
        self.engine.synchronize()
        return {"color16": self.hist[nxt][0].cpu().numpy().view(np.uint16), "surface": self.hist[nxt][1].cpu().numpy().view(np.uint32),
                "resolved8": self.resolved.cpu().numpy(), "motion": self.motion.cpu().numpy()}


@pytest.mark.parametrize("max_history", (4, 32))
@pytest.mark.parametrize("pair", uc.PAIRS, ids=lambda p: "%dx%d-%dx%d" % p)
def test_kernel_matches_definition(vrt, oracle, engine, pair, max_history):
    """Six frames of the pair's moving sequence: every output plane of vrt_upsample equals the numpy definition on the same
    planes, bit for bit, the history out of frame k feeding frame k + 1 on both sides, history_in NULL on frame 0; the class
    shares hold on the GPU's own output (the classes are a function of the planes that were just compared)."""
    pushes, frames = sequence(vrt, oracle, pair)
    g = Gpu(vrt, engine, pair)
    hist, results = None, []
    for k, push in enumerate(pushes):
        prev = pushes[k - 1] if k else pushes[0]
        got = g.step(push, prev, frames[k], max_history)
        exp = ref.upsample(*pair, push, prev, *frames[k], hist, max_history)
        assert ref.same(got, exp) == [], (k, ref.same(got, exp))
        # the classes of the GPU's own output: the definition fed with the GPU's history gives the same planes, hence the same classes
        results.append(exp)
        hist = (got["color16"], got["surface"])
    if pair in uc.SHARED:
        sh = uc.class_shares(results)
        assert uc.shares_hold(pair, sh), sh
        assert max_history == 1 or ((got["surface"][..., 3] >> 24) > 1).any()


def test_optional_outputs(vrt, oracle, engine):
    """With resolved8 and motion NULL the history is what it is with both, and the planes left out are not touched."""
    pair = (45, 30, 67, 45)
    pushes, frames = sequence(vrt, oracle, pair)
    full, bare = Gpu(vrt, engine, pair), Gpu(vrt, engine, pair)
    for k in range(3):
        want = full.step(pushes[k], pushes[max(k - 1, 0)], frames[k])
        got = bare.step(pushes[k], pushes[max(k - 1, 0)], frames[k], resolved=False, motion=False)
    assert ref.same(got, want, ("color16", "surface")) == []
    assert (got["resolved8"] == 0x5A).all() and (got["motion"] == 123.0).all()
    assert (want["resolved8"] != 0x5A).any() and (want["motion"] != 123.0).any()


def _fly(r, frames, mouse=2.0, forward=0.1, strafe=0.5):
    for _ in range(frames):
        r.camera.mouse(mouse, 0.0)
        r.update(1.0 / 60.0, forward, strafe)
        push = r.push_constants()
        yield push, r.render()


def test_frame_graph(vrt, oracle, engine):
    """VoxelRenderer(temporal=True, reproject=True, upsample=True) over 5 moving, jittered frames at 48 x 32 -> 96 x 64 equals the
    definition fed with the renderer's own planes (denoised colour, gBuffer position and normal), upscaler.motion holds the
    definition's vectors and gBuffer.motion stays 0; upsample=False is byte-identical to a renderer constructed without the
    argument; the flag without reproject, or with a shard, raises ValueError."""
    target = (96, 64)
    vol, pal, sky, noise = rc.scene_of(vrt, 1)
    sc = vrt.VoxelScene.from_dense(engine, vol, pal, sky=sky, noise=noise)
    st = vrt.VoxelRenderSettings(targetResolution=target)
    st.fsrSetttings.scaling = vrt.FsrScaling.PERFORMANCE
    st.occlusionSettings.numSamples = 2
    assert st.renderResolution() == (48, 32)
    pair = (48, 32) + target
    r = vrt.VoxelRenderer(engine, st, sc, temporal=True, reproject=True, upsample=True)
    den = vrt.DenoiserStage(engine, st)
    r.camera.position = np.array([12.3, 20.2, -6.0], np.float32); r.camera.updateDirectionVectors()
    hist, prev, moved = None, None, 0.0
    for f, (push, img) in enumerate(_fly(r, 5)):
        engine.synchronize()
        got = img.cpu().numpy().copy()
        gb = r.gBuffer
        color = den.record(gb.color, gb.normal, gb.position).cpu().numpy()
        pl = gb.numpy()
        exp = ref.upsample(*pair, push, prev if prev is not None else push, color, pl["position"], pl["normal8"], hist)
        hist, prev = (exp["color16"], exp["surface"]), push
        assert got.shape == (target[1], target[0], 4) and (got == exp["resolved8"]).all(), f
        assert (r.upscaler.motion.cpu().numpy().view(np.uint32) == exp["motion"].view(np.uint32)).all(), f
        assert gb.motion.shape[:2] == (32, 48) and not gb.motion.any()
        h16, hs = r.upscaler.history()
        assert (h16 == exp["color16"]).all() and (hs == exp["surface"]).all()
        moved = max(moved, float(np.abs(exp["motion"]).max()))
    assert moved > 1.0 and ((exp["surface"][..., 3] >> 24) == 5).any()
    r.upscaler.reset()
    push, img = next(_fly(r, 1))
    engine.synchronize()
    assert ((r.upscaler.history()[1][..., 3] >> 24) == 1).all()
    # upsample=False: today's behaviour exactly
    imgs = []
    for kw in (dict(), dict(upsample=False)):
        r0 = vrt.VoxelRenderer(engine, st, sc, temporal=True, reproject=True, **kw)
        assert r0.upsample is False
        r0.camera.position = np.array([12.3, 20.2, -6.0], np.float32); r0.camera.updateDirectionVectors()
        imgs.append([(img.cpu().numpy().copy(), r0.gBuffer.motion.cpu().numpy().copy()) for _, img in _fly(r0, 3)])
    for (a, ma), (b, mb) in zip(*imgs):
        assert a.tobytes() == b.tobytes() and ma.tobytes() == mb.tobytes()
    with pytest.raises(ValueError):
        vrt.VoxelRenderer(engine, st, sc, temporal=True, upsample=True)
    with pytest.raises(ValueError):
        r.recordCommands(vrt._capi.Shard(0, 2, 16))


def test_cpp_app_upsample_matches_python(vrt, oracle, engine, tmp_path):
    """vrt_app --temporal --reproject --upsample --fly ... --frames 4: the C++ mirror's image equals, byte for byte, the Python
    stages run over the four push blocks the app itself computed."""
    assert os.path.exists(APP), "build with __graft_entry__.build()"
    vol, pal, sky, noise = rc.scene_of(vrt, 1)
    dense = tmp_path / "scene.vrtd"
    _write_dense(dense, vol, pal, sky, noise)
    raw, pushf = tmp_path / "out.rgba", tmp_path / "pushes.bin"
    r = subprocess.run([APP, "--dense", str(dense), "--width", "160", "--height", "96", "--pos", "12.3", "20.2", "-6", "--ao", "2",
                        "--temporal", "--reproject", "--upsample", "--fly", "0.1", "0.5", "2.0", "--frames", "4", "--raw", str(raw),
                        "--dump-pushes", str(pushf)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    blob = pushf.read_bytes()
    assert len(blob) == 4 * 96
    pushes = [vrt._capi.Push.from_buffer_copy(blob[96 * k: 96 * k + 96]) for k in range(4)]
    st = vrt.VoxelRenderSettings(targetResolution=(160, 96))
    st.occlusionSettings.numSamples = 2
    assert tuple(pushes[0].screen_size) == st.renderResolution() == (94, 56)
    sc = vrt.VoxelScene.from_dense(engine, vol, pal, sky=sky, noise=noise)
    geo, den, up = vrt.GeometryStage(engine, st, sc), vrt.DenoiserStage(engine, st), vrt.UpscalerStage(engine, st)
    for p in pushes:
        gb = geo.record(p)
        img = up.record_upsampled(den.record(gb.color, gb.normal, gb.position), gb, p)
    engine.synchronize()
    got = np.frombuffer(raw.read_bytes(), np.uint8).reshape(96, 160, 4)
    assert (got == img.cpu().numpy()).all(), int((got != img.cpu().numpy()).sum())
    assert up.history()[1].shape == (96, 160, 4) and ((up.history()[1][..., 3] >> 24) == 4).any()
    r = subprocess.run([APP, "--dense", str(dense), "--temporal", "--upsample"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--reproject" in r.stderr


def test_reproject_is_unchanged(vrt, oracle, engine):
    """One 96 x 64 sequence through vrt_reproject still matches tests/reproject_reference.py bit for bit."""
    import torch
    W, H = 96, 64
    pushes = rc.pushes_of(vrt, oracle, W, H)
    frames = rc.oracle_frames(vrt, oracle, 1, pushes)
    dev, cap = engine.torch_device, vrt._capi
    hist = [(torch.zeros((H, W, 4), dtype=torch.int16, device=dev), torch.zeros((H, W, 4), dtype=torch.int32, device=dev)) for _ in range(2)]
    resolved = torch.zeros((H, W, 4), dtype=torch.uint8, device=dev); motion = torch.zeros((H, W, 2), dtype=torch.float32, device=dev)
    exp_hist = None
    for k, push in enumerate(pushes):
        prev = pushes[k - 1] if k else pushes[0]
        c, p, n = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in frames[k])
        hin = cap.History(hist[(k - 1) % 2][0].data_ptr(), hist[(k - 1) % 2][1].data_ptr()) if k else None
        hout = cap.History(hist[k % 2][0].data_ptr(), hist[k % 2][1].data_ptr())
        st = vrt.ReprojectSettings().to_c(push)
        cap.check(vrt.lib().vrt_reproject(engine.ctx, W, H, C.byref(push), C.byref(prev), C.byref(st), c.data_ptr(), p.data_ptr(), n.data_ptr(),
                                          C.byref(hin) if hin is not None else None, C.byref(hout), resolved.data_ptr(), motion.data_ptr()))
        engine.synchronize()
        got = {"color16": hist[k % 2][0].cpu().numpy().view(np.uint16), "surface": hist[k % 2][1].cpu().numpy().view(np.uint32),
               "resolved8": resolved.cpu().numpy(), "motion": motion.cpu().numpy()}
        exp = rref.reproject(W, H, push, prev, *frames[k], exp_hist)
        assert rref.same(got, exp) == [], k
        exp_hist = (exp["color16"], exp["surface"])
