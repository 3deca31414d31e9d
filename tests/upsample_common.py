"""Shared by tests/test_upsample_cpu.py, tests/test_gpu_upsample.py and tests/golden/make_upsample_fixtures.py: the size pairs
temporal upsampling is tested on, their sequences -- reproject_common's moving camera over floating_cubes(40, seed, count=50), six
frames, jittered with the Halton sequence of the pair's OWN ratio -- and the definition (tests/upsample_reference.py) run along a
sequence with ping-pong."""
import numpy as np

import reproject_common as rc
import upsample_reference as ref

# (w, h, TW, TH): the smallest sizes at which each part can go wrong
PAIRS = [(64, 43, 96, 64),      # 1.5x
         (56, 37, 96, 64),      # 1.7x, what VoxelRenderSettings._scale gives
         (48, 32, 96, 64),      # 2x
         (32, 21, 96, 64),      # 3x
         (45, 30, 67, 45),      # ragged: partly filled waves, odd rows
         (65, 3, 130, 3),       # three waves per row, rows below a workgroup; x-only jitter as the reproject tests do
         (96, 64, 96, 64),      # ratio 1
         (1, 1, 1, 1)]
MAX_HISTORIES = rc.MAX_HISTORIES
FRAMES = rc.FRAMES
# the pairs the class-share condition is asserted on (the thin and the 1 x 1 pair are exempt, as in the reproject tests)
SHARED = [p for p in PAIRS if p[2] * p[3] >= 256 and p[3] > 3]
NEEDED = rc.NEEDED
# The first scene seed of pick_scene_seed for each pair of SHARED, found on a CPU by the definition's output alone
# (tests/test_upsample_cpu.py::test_class_shares_and_committed_seed checks that the picker still returns them).
SEEDS = {(64, 43, 96, 64): 1, (56, 37, 96, 64): 1, (48, 32, 96, 64): 1, (32, 21, 96, 64): 1, (45, 30, 67, 45): 1, (96, 64, 96, 64): 1}


def pushes_of(vrt, oracle, pair, frames=FRAMES):
    """The push blocks of the sequence rendered at w x h for a display of TW x TH: frame f + 1, the jitter of phase f of the
    8 (TW / w)^2 phases, the camera after f steps of reproject_common's path."""
    w, h, TW, TH = pair
    thin = h <= 3
    path, start = (rc.PATH_THIN, rc.START_THIN) if thin else (rc.PATH, rc.START)
    cam = vrt.CameraController(**start)
    out = []
    for f in range(frames):
        if f:
            cam.mouse(path["mouseX"], path["mouseY"])
            cam.update(1.0 / 60.0, path["forward"], path["strafe"])
        j = oracle.jitter(f, w, TW)[1:]
        if thin:
            j = (j[0], 0.0)                 # reproject_common.pushes_of says why
        out.append(vrt.make_push(cam, (rc.N_SCENE,) * 3, (w, h), f + 1, j))
    return out


def run_definition(pair, pushes, frames, max_history=32, tol_abs=0.5, tol_rel=None, hist=None):
    """The definition along the sequence: frame k's history feeds frame k + 1.  Returns the list of per-frame result dicts."""
    w, h, TW, TH = pair
    out = []
    for k, (c, p, n) in enumerate(frames):
        r = ref.upsample(w, h, TW, TH, pushes[k], pushes[k - 1] if k else pushes[0], c, p, n, hist, max_history, tol_abs, tol_rel)
        hist = (r["color16"], r["surface"])
        out.append(r)
    return out


def class_shares(results):
    """Shares of the pixel classes, and of sampled / carried, over the frames that had a history (all but the first)."""
    cls = np.concatenate([r["cls"].ravel() for r in results[1:]])
    alpha = np.concatenate([r["alpha"].ravel() for r in results[1:]])
    return ref.shares(cls, alpha)


def shares_hold(pair, sh):
    """The class-share condition: every class at >= 5 % of the pixels; where the display is larger than the frame (every such pair
    here has a ratio of 1.5 or more along x or y) also the pixels with history whose sample counted (sampled) and those that carried
    their history on (carried), at ratio 1 -- where every sample falls within half a pixel of its own pixel, so nothing is carried,
    and where the other classes make sampled >= 90 % of ALL pixels impossible -- sampled >= 90 % of the pixels with history
    instead."""
    ok = min(sh[k] for k in NEEDED) >= 0.05
    if (pair[0], pair[1]) != (pair[2], pair[3]):
        return ok and sh["sampled"] >= 0.05 and sh["carried"] >= 0.05
    return ok and sh["sampled"] >= 0.9 * (sh["full"] + sh["partial"])


def pick_scene_seed(vrt, oracle, pair, first=1, tries=40):
    """The first scene seed whose sequence satisfies shares_hold -- decided on the definition's output alone."""
    pushes = pushes_of(vrt, oracle, pair)
    seen = []
    for seed in range(first, first + tries):
        sh = class_shares(run_definition(pair, pushes, rc.oracle_frames(vrt, oracle, seed, pushes, geometry_only=True)))
        if shares_hold(pair, sh):
            return seed, sh
        seen.append((seed, sh))
    raise AssertionError(f"no scene seed in {first} .. {first + tries - 1} satisfies the class-share condition at {pair}: {seen[:3]} ...")


def seed_of(pair):
    return SEEDS.get(tuple(pair), 1)
