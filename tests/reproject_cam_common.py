"""Shared by tests/test_reproject_cam_cpu.py, tests/test_gpu_reproject_cam.py and tests/golden/make_reproject_cam_fixtures.py: the
moving sequences temporal reprojection for ray cameras is tested on -- floating_cubes(40, seed, count=50) seen by a perspective
camera with a 70-degree field of view, an orthographic one and a panorama -- the oracle's frames over those cameras' rays, and
the definition (tests/reproject_cam_reference.py) run along a sequence with ping-pong.

The paths.  Perspective and orthographic: the strafing, turning path of tests/reproject_common.py (the turn is what uncovers
surfaces in a parallel view, whose translation shifts every depth alike).  Panorama: the camera's orientation is fixed, and a tap
wraps only where the previous-screen position falls into the one column across the seam (the direction -x), so in steady flight
1 / W of the pixels have such a tap.  A twentieth of the pixels need the seam's neighbourhood magnified: the camera dives along
-x at the nearest cube face, covering DIVE of the remaining distance per frame, which spreads that one column over 1 / (1 - DIVE)
columns of the next frame, and climbs SLANT of it, which is what uncovers surfaces."""
import numpy as np

import raygen_reference as rays
import reproject_cam_reference as ref
import reproject_common as rc

SIZES = rc.SIZES
MAX_HISTORIES = rc.MAX_HISTORIES
FRAMES = rc.FRAMES
N_SCENE = rc.N_SCENE
MODELS = ("perspective", "orthographic", "panorama")
FOV_DEG = 70.0
HALF_WIDTH = 14.0
DIVE = 0.9
SLANT = 0.3
NEEDED = {"perspective": ("miss", "full", "partial", "disoccluded", "outside"),
          "orthographic": ("miss", "full", "partial", "disoccluded", "outside"),
          "panorama": ("miss", "full", "partial", "disoccluded", "wrapped")}


def dive_positions(vol, frames=FRAMES):
    """The panorama's path in volume `vol` ([z, y, x] ids): towards -x at the +x face of the solid voxel with the largest x among
    the rows of the volume's middle, DIVE of the remaining distance per frame, and SLANT of it upwards (the azimuthal
    magnification at the seam does not depend on the height, and the climb is what uncovers surfaces)."""
    D, Hh, Ww = vol.shape
    best = None
    for y in range(Hh // 4, 3 * Hh // 4):
        for z in range(D // 4, 3 * D // 4):
            xs = np.nonzero(vol[z, y])[0]
            if len(xs) and xs[-1] < Ww - 4 and (best is None or xs[-1] > best[0]):
                best = (int(xs[-1]), y, z)
    assert best is not None
    face, r, out = best[0] + 1.0, float(Ww) + 8.0 - (best[0] + 1.0), []
    for f in range(frames):
        out.append((face + r, best[1] + 0.3 + SLANT * r, best[2] + 0.7))
        r *= 1.0 - DIVE
    return out


def cameras_of(vrt, oracle, model, W, H, vol=None, frames=FRAMES):
    """The vrt_ray_camera blocks of the sequence at W x H, frame by frame."""
    if model == "panorama":
        return [vrt.RayCamera.panorama(p).to_c((W, H)) for p in dive_positions(vol, frames)]
    pushes = rc.pushes_of(vrt, oracle, W, H, frames)
    out = []
    for p in pushes:
        c = vrt._capi.RayCamera()
        c.model = rays.PERSPECTIVE if model == "perspective" else rays.ORTHOGRAPHIC
        c.basis = vrt._capi.Push.from_buffer_copy(p)
        c.tan_half = float(np.float32(np.tan(np.radians(FOV_DEG) / 2.0)))
        c.half_width = HALF_WIDTH
        if model == "orthographic":
            c.basis.camera_jitter[:] = [0.0, 0.0]
        out.append(c)
    return out


def rays_of(cam, W, H):
    b = cam.basis
    return rays.camera_rays(cam.model, W, H, list(b.cam_pos)[:3], list(b.cam_dir)[:3], list(b.cam_right)[:3], list(b.cam_up)[:3],
                            list(b.camera_jitter), cam.tan_half, cam.half_width)


def oracle_frames(vrt, oracle, seed, cams, W, H, vol=None):
    """[(color8, position, normal8)] of the sequence: every ray of raygen_reference.camera_rays traced by the oracle; position =
    (hit point, 0) and normal8 = the SNORM8 codes of the hit normal, zeros on a miss, as the geometry stage writes them.  The
    colour is a pattern of the material, the pixel and the frame: it changes from frame to frame, which is all the blend needs."""
    if vol is None:
        vol = rc.scene_of(vrt, seed)[0]
    osn = oracle.OracleScene(vol, vrt.synthetic.default_palette())
    out = []
    for f, cam in enumerate(cams):
        o, d = rays_of(cam, W, H)
        pos = np.zeros((H * W, 4), np.float32); nrm = np.zeros((H * W, 4), np.int8); mat = np.zeros(H * W, np.uint32)
        for i in range(H * W):
            h = oracle.trace_ray(osn, o[i], d[i], 512)
            if h.material:
                pos[i, :3] = h.pos[:]
                nrm[i, :3] = [int(np.floor(v * 127.0 + 0.5)) for v in h.normal]
                mat[i] = h.material
        idx = np.arange(H * W, dtype=np.uint32)
        col = np.zeros((H * W, 4), np.uint8)
        for ch in range(3):
            col[:, ch] = ((mat * (37 + 20 * ch) + idx * (3 + ch) + (f + 1) * (41 + 7 * ch)) % 256).astype(np.uint8)
        out.append((col.reshape(H, W, 4), pos.reshape(H, W, 4), nrm.reshape(H, W, 4)))
    return out


def run_definition(W, H, cams, frames, max_history=32, tol_abs=0.5, tol_rel=None):
    """The definition along the sequence: frame k's history feeds frame k + 1.  Returns the list of per-frame result dicts."""
    out, hist = [], None
    for k, (c, p, n) in enumerate(frames):
        r = ref.reproject(W, H, cams[k], cams[k - 1] if k else cams[0], c, p, n, hist, max_history, tol_abs, tol_rel)
        hist = (r["color16"], r["surface"])
        out.append(r)
    return out


def class_shares(results):
    """Shares of the pixel classes, and of the pixels with a wrapped tap, over the frames that had a history (all but the first)."""
    cls = np.concatenate([r["cls"].ravel() for r in results[1:]])
    sh = ref.shares(cls)
    sh["wrapped"] = float(np.concatenate([r["wrapped"].ravel() for r in results[1:]]).mean())
    return sh


_PICKED = {}


def pick_scene_seed(vrt, oracle, model, W, H, first=1, tries=40):
    """(seed, shares, cameras, frames): the first scene seed whose sequence holds every class NEEDED[model] at >= 5 % of the pixels
    that had a history -- decided on the definition's output alone."""
    key = (model, W, H)
    if key in _PICKED:
        return _PICKED[key]
    best = None
    for seed in range(first, first + tries):
        vol = rc.scene_of(vrt, seed)[0]
        cams = cameras_of(vrt, oracle, model, W, H, vol)
        frames = oracle_frames(vrt, oracle, seed, cams, W, H, vol)
        sh = class_shares(run_definition(W, H, cams, frames))
        worst = min(sh[k] for k in NEEDED[model])
        if worst >= 0.05:
            _PICKED[key] = (seed, sh, cams, frames)
            return _PICKED[key]
        if best is None or worst > best[0]:
            best = (worst, seed, sh)
    raise AssertionError(f"{model} {W}x{H}: no scene seed in {first} .. {first + tries - 1} gives 5 % of every class; best {best}")
