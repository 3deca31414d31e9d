"""Temporal upsampling for ray cameras without a GPU: the per-pixel definition (csrc/vrt_upsample_cam.h, compiled for the host by
tests/native/upsample_cam_host.cpp) against its numpy float32 restatement (tests/upsample_cam_reference.py) bit for bit, the
identity with vrt_upsample's definition for the 90-degree pinhole, the panorama's seam, what the pass exists for -- a static camera's
display-resolution image beats the enlargement of one frame and the same sequence without offsets -- and the C-ABI surface of
vrt_upsample_camera."""
import ctypes as C

import numpy as np
import pytest

import reproject_common as rc
import upsample_cam_common as uc
import upsample_cam_reference as ref
import upsample_reference as pin


@pytest.mark.parametrize("size", uc.SIZES, ids=lambda s: "%dx%d-%dx%d" % s)
@pytest.mark.parametrize("model", uc.MODELS)
def test_host_function_matches_numpy_definition(vrt, oracle, model, size):
    """Five frames of a moving camera, the samples offset by vrt_jitter_offset, the frames traced by the oracle over the offset
    rays: color16, surface words, motion bit patterns and resolved8 of the header equal the numpy definition in every frame, each
    side fed its own history."""
    w, h, TW, TH = size
    cams, _, offs, frames, exp = uc.case(vrt, oracle, model, size)
    assert any(o != (0.0, 0.0) for o in offs) or model == "perspective"
    hist = None
    for k, (c, p, n) in enumerate(frames):
        r, got = uc.host_upsample(w, h, TW, TH, cams[k], cams[k - 1] if k else cams[0], c, p, n, hist)
        assert r == 0
        assert ref.same(got, exp[k]) == [], (k, ref.same(got, exp[k]))
        hist = (got["color16"], got["surface"])
        cnt = got["surface"][..., 3] >> 24
        assert cnt.min() >= 1 and cnt.max() <= k + 1
    if w * h >= 256:
        assert (cnt > 1).any() and any(np.abs(e["motion"]).max() > 0.25 for e in exp[1:])


def test_pinhole_identity(vrt, oracle):
    """Perspective with tan_half == 1.0f: every plane of every frame equals vrt_upsample's definition (tests/upsample_reference.py)
    on the same push blocks, jittered, header and numpy restatement both -- although the pass cameras carry no jitter."""
    w, h, TW, TH = 24, 14, 48, 28
    pushes = rc.pushes_of(vrt, oracle, w, h, uc.FRAMES)
    frames = rc.oracle_frames(vrt, oracle, 1, pushes)
    assert any(p.camera_jitter[0] != 0 for p in pushes)
    cams = []
    for p in pushes:
        c = vrt._capi.RayCamera(); c.model = ref.PERSPECTIVE; c.basis = vrt._capi.Push.from_buffer_copy(p); c.tan_half = 1.0
        c.basis.camera_jitter[:] = [0.0, 0.0]
        cams.append(c)
    assert np.float32(uc.host().uch_default_tol_rel(C.byref(cams[0]), w)) == ref.default_tol_rel(cams[0], w) == pin.default_tol_rel(pushes[0], w)
    hist_p = hist_h = hist_n = None
    for k, (c, p, n) in enumerate(frames):
        a, b = k, max(k - 1, 0)
        want = pin.upsample(w, h, TW, TH, pushes[a], pushes[b], c, p, n, hist_p)
        r, got = uc.host_upsample(w, h, TW, TH, cams[a], cams[b], c, p, n, hist_h)
        exp = ref.upsample(w, h, TW, TH, cams[a], cams[b], c, p, n, hist_n)
        assert r == 0 and ref.same(got, want) == [] and ref.same(exp, want) == [], k
        hist_p, hist_h, hist_n = [(x["color16"], x["surface"]) for x in (want, got, exp)]
    assert ((want["surface"][..., 3] >> 24) > 2).any()


def test_pinhole_identity_with_the_upsample_host_program(vrt, oracle, tmp_path_factory, tmp_path):
    """The same identity against the existing host program of csrc/vrt_upsample.h (tests/native/upsample_host.cpp)."""
    import test_upsample_cpu as tu
    exe = tu._build(tmp_path_factory, "upsample_host_for_cam", [])
    w, h, TW, TH = 24, 14, 48, 28
    pushes = rc.pushes_of(vrt, oracle, w, h, uc.FRAMES)
    frames = rc.oracle_frames(vrt, oracle, 1, pushes)
    out = tu.run_host(exe, tmp_path, (w, h, TW, TH), pushes, frames)
    hist = None
    for k, (c, p, n) in enumerate(frames):
        cams = []
        for q in (pushes[k], pushes[max(k - 1, 0)]):
            cc_ = vrt._capi.RayCamera(); cc_.model = ref.PERSPECTIVE; cc_.basis = vrt._capi.Push.from_buffer_copy(q); cc_.tan_half = 1.0
            cams.append(cc_)
        r, got = uc.host_upsample(w, h, TW, TH, cams[0], cams[1], c, p, n, hist)
        assert r == 0 and ref.same(got, out[k]) == [], k
        hist = (got["color16"], got["surface"])


def test_seam_static_camera(vrt, oracle):
    """Panorama at 32x16 -> 64x32 inside the closed room, the camera at rest, offsets on: every hit pixel's motion is exactly 0,
    display columns 0 and TW - 1 reach a count above 1 within four frames, and at least one sample whose ux lies beyond TW - 1
    has a non-zero weight for column 0 (S1).  The offsets are chosen for that: vrt_jitter_offset's stay within half a render pixel,
    which at this width (w = 32 < 180) carries no sample of render column 0 across the seam -- at production widths it does, see
    tests/test_raygen_offset_cpu.py and DESIGN.md 8; uc.SEAM_OFFSETS push it 0.6 and 0.7 render pixels left."""
    w, h, TW, TH = uc.SEAM
    cams, _, offs, frames, exp = uc.case(vrt, oracle, "panorama", uc.SEAM, moving=False, frames=4, offset_list=uc.SEAM_OFFSETS)
    seam = 0
    for k, e in enumerate(exp):
        assert (frames[k][2].view(np.uint8).reshape(h, w, 4)[..., :3] != 0).any(axis=-1).all()          # the room is closed
        assert (e["motion"] == 0).all(), k
        seam += int((e["seam_alpha"][:, 0] & (e["ux"][:, 0] > TW - 1)).sum())
        r, got = uc.host_upsample(w, h, TW, TH, cams[k], cams[max(k - 1, 0)], *frames[k], hist=(exp[k - 1]["color16"], exp[k - 1]["surface"]) if k else None)
        assert r == 0 and ref.same(got, e) == [], k
    cnt = exp[-1]["surface"][..., 3] >> 24
    # (not every row: a display pixel on the edge between two surfaces restarts when its sample shows the other one)
    assert (cnt[:, 0] > 1).any() and (cnt[:, TW - 1] > 1).any() and (cnt[:, [0, TW - 1]] > 1).mean() > 0.5
    print(f"\nsamples beyond column TW - 1 with weight for column 0: {seam}")
    assert seam > 0


def test_seam_moving_camera(vrt, oracle):
    """The camera sliding past the seam direction: at least one pixel takes a history tap through the wrap (S3 / S4), and the header
    agrees with the definition there."""
    w, h, TW, TH = uc.SEAM
    cams, _, offs, frames, exp = uc.case(vrt, oracle, "panorama", uc.SEAM, slide=0.45)
    wrapped = sum(int(e["wrapped"].sum()) for e in exp)
    print(f"\npixels with a tap through the wrap: {wrapped}")
    assert wrapped > 0
    hist = None
    for k, (c, p, n) in enumerate(frames):
        r, got = uc.host_upsample(w, h, TW, TH, cams[k], cams[max(k - 1, 0)], c, p, n, hist)
        assert r == 0 and ref.same(got, exp[k]) == [], k
        hist = (got["color16"], got["surface"])


@pytest.mark.parametrize("model,wave", (("orthographic", 1.5), ("panorama", 0.36)))
def test_offsets_resolve_what_one_frame_cannot(vrt, oracle, model, wave):
    """What the pass exists for.  A camera at rest over one full jitter period: the resolved display-resolution image is nearer (mean
    absolute code error) to the oracle's G-buffer drawn directly at TW x TH from the same camera than the nearest-sample
    enlargement of one render-resolution frame is, and nearer than the same sequence run with offsets of 0.  Every image is
    uc.surface_colour of its G-buffer: a wave along the surfaces of about 3.5 render pixels (wave: radians per voxel -- a render
    pixel of the orthographic view spans 1.2 voxels, one of the panorama about 5 on the room's walls).  Both baselines are computed
    here; no fixed threshold."""
    w, h, TW, TH = 24, 14, 48, 28
    phases = int(vrt.lib().vrt_jitter_phase_count(w, TW))
    vol = uc.volume_of(vrt, model)
    osn = oracle.OracleScene(vol, vrt.synthetic.default_palette())
    err = {}
    for offsets in (True, False):
        cams, raycams, offs = uc.sequence(vrt, oracle, model, w, h, TW, frames=phases, moving=False, offsets=offsets)
        frames = uc.oracle_frames(vrt, oracle, vol, raycams, offs, w, h, shade=wave)
        res = uc.run_definition(w, h, TW, TH, cams, frames, max_history=phases)
        # the images compared below are the HEADER's: its rays are the rays traced, and its planes along the same sequence, fed its
        # own history, equal the definition's bit for bit
        hist = None
        for k, (c, p, n) in enumerate(frames):
            rr, ho, hd = uc.host_rays_offset(raycams[k], w, h, offs[k])
            eo, ed = ref.camera_rays_offset(raycams[k], w, h, offs[k])
            assert rr == 0 and (ho.view(np.uint32) == eo.view(np.uint32)).all() and (hd.view(np.uint32) == ed.view(np.uint32)).all(), k
            rr, got = uc.host_upsample(w, h, TW, TH, cams[k], cams[max(k - 1, 0)], c, p, n, hist, max_history=phases)
            assert rr == 0 and ref.same(got, res[k]) == [], (k, ref.same(got, res[k]))
            hist = (got["color16"], got["surface"])
        res[-1] = dict(res[-1], resolved8=got["resolved8"])
        if offsets:
            o, d = ref.camera_rays_offset(cams[0], TW, TH, (0.0, 0.0))
            pos, nrm, _ = uc.trace(oracle, osn, o, d, TW, TH)
            truth = uc.surface_colour(pos, nrm, wave)[..., :3].astype(np.int64)
            ry, rx = pin.source(w, h, TW, TH)
            zero = uc.oracle_frames(vrt, oracle, vol, raycams[:1], [(0.0, 0.0)], w, h, shade=wave)[0][0]
            err["nearest"] = float(np.abs(zero[ry, rx][..., :3].astype(np.int64) - truth).mean())
        err["offsets" if offsets else "no offsets"] = float(np.abs(res[-1]["resolved8"][..., :3].astype(np.int64) - truth).mean())
    print(f"\n{model}: mean absolute code error {err}")
    assert err["offsets"] < err["nearest"] and err["offsets"] < err["no offsets"], err


def _cam(vrt, model, res=(48, 32), tan_half=1.0, half_width=10.0):
    c = vrt._capi.RayCamera()
    c.model = model
    c.basis = vrt.make_push(vrt.CameraController(position=(20.3, 20.2, -14.0), yaw=90.0, pitch=0.0), (40, 40, 40), res, 0, (0.0, 0.0))
    c.tan_half, c.half_width = tan_half, half_width
    return c


class _World:
    """A complete, valid argument list of vrt_upsample_camera or vrt_upsample over fake memory (never dereferenced)."""

    def __init__(self, vrt, name):
        cap = vrt._capi
        self.lib, self.name = vrt.lib(), name
        self.w, self.h, self.TW, self.TH = 48, 32, 96, 64
        n, tn = self.w * self.h, self.TW * self.TH
        sizes = dict(col=4 * n, pos=16 * n, nrm=4 * n, hin_c=8 * tn, hin_s=16 * tn, hout_c=8 * tn, hout_s=16 * tn, res=4 * tn, mot=8 * tn)
        self._buf = (C.c_uint8 * (sum(sizes.values()) + 64 * 12))()
        o = (C.addressof(self._buf) + 63) & ~63
        at = {}
        for k, v in sizes.items():
            at[k] = o
            o += v + 64
        cur = _cam(vrt, ref.PERSPECTIVE, (self.w, self.h))
        if name == "vrt_upsample":
            cur = cur.basis
        self.base = dict(ctx=C.c_void_p(at["col"]), w=self.w, h=self.h, TW=self.TW, TH=self.TH, cur=cur, prev=cur,
                         st=cap.ReprojectSettings(32, 0.5, 0.1), col=at["col"], pos=at["pos"], nrm=at["nrm"],
                         hin=cap.History(at["hin_c"], at["hin_s"]), hout=cap.History(at["hout_c"], at["hout_s"]), res=at["res"], mot=at["mot"])

    def call(self, **kw):
        a = dict(self.base); a.update(kw)
        r_ = lambda x: C.byref(x) if x is not None else None
        rc_ = getattr(self.lib, self.name)(a["ctx"], a["w"], a["h"], a["TW"], a["TH"], r_(a["cur"]), r_(a["prev"]), r_(a["st"]), a["col"], a["pos"],
                                           a["nrm"], r_(a["hin"]), r_(a["hout"]), a["res"], a["mot"])
        return int(rc_), self.lib.vrt_last_error().decode()


def test_c_abi_surface(vrt):
    """Every VRT_ERR_INVALID and VRT_ERR_UNSUPPORTED of vrt_upsample_camera, answered before a context or a device is looked at
    (there is none here) under the function's name; the rules shared with vrt_upsample give the same code for the same broken
    call, and for a pair of broken rules the rule vrt_upsample reports first."""
    cap = vrt._capi
    for name in ("vrt_upsample_camera", "vrt_upsample_camera_settings_default", "vrt_camera_rays_offset"):
        assert name in cap.SYMBOLS and hasattr(C.CDLL(cap.LIB_PATH), name)
    assert C.sizeof(cap.RayCamera) == uc.host().uch_sizeof_camera()
    INVALID, UNSUPPORTED = 1, 7
    x = _World(vrt, "vrt_upsample_camera")
    u = _World(vrt, "vrt_upsample")
    u.base = dict(x.base, cur=u.base["cur"], prev=u.base["prev"])           # the same fake memory: one replacement serves both
    H_, S_ = cap.History, cap.ReprojectSettings
    hin, hout, b = x.base["hin"], x.base["hout"], x.base
    nan, inf = float("nan"), float("inf")
    shared = [
        (dict(ctx=None), "NULL"), (dict(cur=None), "NULL"), (dict(prev=None), "NULL"), (dict(col=None), "NULL"), (dict(pos=None), "NULL"),
        (dict(nrm=None), "NULL"), (dict(hout=None), "NULL"), (dict(hout=H_(None, hout.surface)), "NULL"), (dict(hin=H_(hin.color16, None)), "NULL"),
        (dict(w=0), "size"), (dict(h=-1), "size"), (dict(TW=0), "size"), (dict(TW=40000), "size"), (dict(TW=47), "smaller"), (dict(TH=31), "smaller"),
        (dict(TW=16384, TH=16384), "2^28"),
        (dict(st=S_(0, 0.5, 0.1)), "max_history"), (dict(st=S_(256, 0.5, 0.1)), "max_history"), (dict(st=S_(32, -0.5, 0.1)), "tolerance"),
        (dict(st=S_(32, 0.5, nan)), "tolerance"), (dict(st=S_(32, inf, 0.1)), "tolerance"),
        (dict(hout=hin), "overlap"), (dict(hout=H_(hin.color16, hout.surface)), "overlap"), (dict(res=b["col"]), "overlap"), (dict(mot=hin.surface), "overlap"),
        (dict(pos=b["pos"] + 4), "aligned"), (dict(mot=b["mot"] + 4), "aligned"), (dict(res=b["res"] + 2), "aligned"),
    ]
    for kw, word in shared:
        code, msg = x.call(**kw)
        ucode, umsg = u.call(**kw)
        assert code == (UNSUPPORTED if word == "2^28" else INVALID) and word in msg and msg.startswith("vrt_upsample_camera:"), (kw, msg)
        assert code == ucode and word in umsg, (kw, msg, umsg)
    # pairs of broken rules: the first one of vrt_upsample's order -- NULL, size, settings, cameras, planes
    order = [dict(col=None), dict(TW=47), dict(st=S_(0, 0.5, 0.1)), dict(hout=hin)]
    words = ["NULL", "smaller", "max_history", "overlap"]
    for i in range(len(order)):
        for j in range(i + 1, len(order)):
            kw = dict(order[i]); kw.update(order[j])
            code, msg = x.call(**kw)
            ucode, umsg = u.call(**kw)
            assert words[i] in msg and words[i] in umsg and code == ucode, (kw, msg, umsg)
    bad_cam = _cam(vrt, ref.ORTHOGRAPHIC, half_width=0.0)
    assert "max_history" in x.call(st=S_(0, 0.5, 0.1), cur=bad_cam, prev=bad_cam)[1]
    assert "current camera" in x.call(cur=bad_cam, prev=bad_cam, hout=hin)[1]
    # the pass's own camera rules
    cams = {m: _cam(vrt, m) for m in (ref.PERSPECTIVE, ref.ORTHOGRAPHIC, ref.PANORAMA)}
    for a, c in ((ref.PERSPECTIVE, ref.ORTHOGRAPHIC), (ref.PANORAMA, ref.PERSPECTIVE), (ref.ORTHOGRAPHIC, ref.PANORAMA)):
        code, msg = x.call(cur=cams[a], prev=cams[c])
        assert code == INVALID and "different models" in msg

    def bad_cams():
        yield _cam(vrt, 3), True
        yield _cam(vrt, -1), True
        for th_ in (0.0, -1.0, nan, inf):
            yield _cam(vrt, ref.PERSPECTIVE, tan_half=th_), False
            yield _cam(vrt, ref.ORTHOGRAPHIC, half_width=th_), False
        for m in (ref.PERSPECTIVE, ref.ORTHOGRAPHIC):
            c = _cam(vrt, m); c.basis.cam_right[:] = [0.0, 0.0, 0.0, 0.0]; yield c, False
            c = _cam(vrt, m); c.basis.cam_up[1] = inf; yield c, False
        for m in (ref.PERSPECTIVE, ref.ORTHOGRAPHIC, ref.PANORAMA):
            c = _cam(vrt, m); c.basis.cam_pos[2] = nan; yield c, False
        c = _cam(vrt, ref.PERSPECTIVE); c.basis.camera_jitter[0] = inf; yield c, False

    for bad, both in bad_cams():
        good = cams.get(bad.model, bad)
        if both:
            code, msg = x.call(cur=bad, prev=bad)
            assert code == INVALID and "camera" in msg and msg.startswith("vrt_upsample_camera:")
            continue
        code, msg = x.call(cur=bad, prev=good)
        assert code == INVALID and "current camera" in msg, msg
        code, msg = x.call(cur=good, prev=bad)
        assert code == INVALID and "previous camera" in msg, msg
    # a basis that passes raygen_consts_of's double determinant but whose fp32 determinant underflows to 0
    for m in (ref.PERSPECTIVE, ref.ORTHOGRAPHIC):
        tiny = _cam(vrt, m)
        tiny.basis.cam_right[:] = [1e-25, 0.0, 0.0, 0.0]; tiny.basis.cam_up[:] = [0.0, -1e-25, 0.0, 0.0]; tiny.basis.cam_dir[:] = [0.0, 0.0, 1.0, 0.0]
        code, msg = x.call(cur=tiny, prev=cams[m])
        assert code == INVALID and "current camera's basis is degenerate" in msg, msg
        code, msg = x.call(cur=cams[m], prev=tiny)
        assert code == INVALID and "previous camera's basis is degenerate" in msg, msg
    # the defaults are vrt_reproject_camera's at the render width
    st, st2 = cap.ReprojectSettings(), cap.ReprojectSettings()
    for m, cam in cams.items():
        vrt.lib().vrt_upsample_camera_settings_default(C.byref(cam), 48, C.byref(st))
        vrt.lib().vrt_reproject_camera_settings_default(C.byref(cam), 48, C.byref(st2))
        assert (st.max_history, st.tol_abs, st.tol_rel) == (32, 0.5, st2.tol_rel) and np.float32(st.tol_rel) == ref.default_tol_rel(cam, 48)
    assert callable(vrt.UpscalerStage.record_upsampled_camera)
