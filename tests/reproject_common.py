"""Shared by tests/test_reproject_cpu.py, tests/test_gpu_reproject.py and tests/golden/make_reproject_fixtures.py: the moving-camera
sequences temporal reprojection is tested on -- floating_cubes(40, seed, count=50) seen by a camera that strafes, turns and is
jittered -- and the definition (tests/reproject_reference.py) run along a sequence with ping-pong."""
import numpy as np

import reproject_reference as ref

SIZES = [(96, 64), (67, 45), (130, 3), (1, 1)]
MAX_HISTORIES = (1, 4, 32, 255)
FRAMES = 6
N_SCENE = 40
# per frame: cursor motion in pixels (= degrees of yaw / pitch, camera_controller.cpp:46-68) and the forward / strafe axes at
# delta = 1 / 60 (50 voxels per second): a turn of 9 degrees and a strafe of 1.7 voxels per frame, from inside the cloud of
# cubes -- fast enough that a twentieth of the pixels leave the frame, near enough that parallax uncovers as many
PATH = dict(mouseX=9.0, mouseY=-0.1, forward=0.5, strafe=2.0)
START = dict(position=(10.3, 20.2, 2.0), yaw=100.0, pitch=2.0)
# a frame of three rows spans 1.4 degrees of pitch: the same path without its pitch, or every row would leave the frame
PATH_THIN = dict(PATH, mouseY=0.0)
START_THIN = dict(START, pitch=0.0)


def pushes_of(vrt, oracle, W, H, frames=FRAMES, jittered=True, path=None, start=None):
    """The push blocks of the sequence at W x H: frame f + 1, the Halton jitter of a 1.7x upscale, the camera after f steps."""
    path = path or (PATH_THIN if H <= 3 else PATH)
    start = start or (START_THIN if H <= 3 else START)
    cam = vrt.CameraController(**start)
    out = []
    for f in range(frames):
        if f:
            cam.mouse(path["mouseX"], path["mouseY"])
            cam.update(1.0 / 60.0, path["forward"], path["strafe"])
        j = oracle.jitter(f, max(W, 2), int(max(W, 2) * 1.7))[1:] if jittered else (0.0, 0.0)
        if H <= 3:
            # cameraJitter enters the ray in WORLD y as jitter / H * 2 (voxel_volume.frag:319): half a pixel of a three-row frame
            # turns the view by 5 degrees, four times the frame's height -- the thin frames are jittered along x only
            j = (j[0], 0.0)
        out.append(vrt.make_push(cam, (N_SCENE,) * 3, (W, H), f + 1, j))
    return out


def scene_of(vrt, seed):
    vol = vrt.synthetic.floating_cubes(N_SCENE, seed=seed, count=50)
    pal = vrt.synthetic.default_palette(metallic_ids=range(200, 256))
    return vol, pal, vrt.synthetic.sky_gradient(64, 32), vrt.synthetic.blue_noise_standin(64)


def oracle_frames(vrt, oracle, seed, pushes, geometry_only=False):
    """[(color8, position, normal8)] of the sequence by the oracle: the colour is the rendered one (reference defaults with 2 AO
    samples, so that it changes from frame to frame), or with geometry_only zeros (class shares need none)."""
    vol, pal, sky, noise = scene_of(vrt, seed)
    osn = oracle.OracleScene(vol, pal, sky=sky, noise=noise)
    st = vrt.VoxelRenderSettings.primary_only() if geometry_only else vrt.VoxelRenderSettings()
    if not geometry_only:
        st.occlusionSettings.numSamples = 2
    pr = oracle.params_from(st.to_c())
    out = []
    for p in pushes:
        fr = oracle.render(osn, p, pr, planes=["normal8", "position"] if geometry_only else ["color8", "normal8", "position"], nthreads=8)
        out.append((fr["color8"] if not geometry_only else np.zeros(fr["normal8"].shape, np.uint8), fr["position"], fr["normal8"]))
    return out


def run_definition(W, H, pushes, frames, max_history=32, tol_abs=0.5, tol_rel=None):
    """The definition along the sequence: frame k's history feeds frame k + 1.  Returns the list of per-frame result dicts."""
    out, hist = [], None
    for k, (c, p, n) in enumerate(frames):
        r = ref.reproject(W, H, pushes[k], pushes[k - 1] if k else pushes[0], c, p, n, hist, max_history, tol_abs, tol_rel)
        hist = (r["color16"], r["surface"])
        out.append(r)
    return out


def class_shares(results):
    """Shares of the pixel classes over the frames that had a history (all but the first)."""
    cls = np.concatenate([r["cls"].ravel() for r in results[1:]])
    return ref.shares(cls)


NEEDED = ("miss", "full", "partial", "disoccluded", "outside")


def pick_scene_seed(vrt, oracle, W, H, first=1, tries=40):
    """A scene seed whose sequence holds misses, pixels with full history, partially valid pixels, disoccluded hits and
    projections outside the frame at >= 5 % of the pixels each -- decided on the definition's output alone."""
    pushes = pushes_of(vrt, oracle, W, H)
    best = None
    for seed in range(first, first + tries):
        sh = class_shares(run_definition(W, H, pushes, oracle_frames(vrt, oracle, seed, pushes, geometry_only=True)))
        if min(sh[k] for k in NEEDED) >= 0.05:
            return seed, sh
        if best is None or min(sh[k] for k in NEEDED) > min(best[1][k] for k in NEEDED):
            best = (seed, sh)
    raise AssertionError(f"no scene seed in {first} .. {first + tries - 1} gives 5 % of every class at {W}x{H}; best {best}")
