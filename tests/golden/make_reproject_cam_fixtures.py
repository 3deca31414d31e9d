"""Writes tests/golden/render_reproject_cam.npz: per camera model two 12 x 10 frames of the moving sequences of
tests/reproject_cam_common.py (the oracle's planes over the cameras' rays, and the vrt_ray_camera blocks) and what the definition
of temporal reprojection for ray cameras (tests/reproject_cam_reference.py) makes of them -- history, resolved image and motion of
both frames.  It pins the DEFINITION between rounds: tests/test_reproject_cam_cpu.py checks that today's header and today's numpy
restatement both reproduce it bit for bit.  Regenerate only on purpose: python tests/golden/make_reproject_cam_fixtures.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import voxel_raytracing_amd as vrt                     # host-side helpers only (synthetic scenes, camera); no GPU needed
from oracle import oracle
import reproject_cam_common as cc
import reproject_cam_reference as ref
import reproject_common as rc

HERE = os.path.dirname(os.path.abspath(__file__))
W, H, SEED, MAX_HISTORY = 12, 10, 3, 32


def main():
    keep = {"max_history": np.array(MAX_HISTORY, np.uint32), "size": np.array([W, H], np.int32)}
    vol = rc.scene_of(vrt, SEED)[0]
    for model in cc.MODELS:
        # (the panorama's third and fourth pose: the dive's first step is so long that nothing of frame 0 survives it)
        cams = cc.cameras_of(vrt, oracle, model, W, H, vol, frames=4)[2:] if model == "panorama" else cc.cameras_of(vrt, oracle, model, W, H, vol, frames=2)
        frames = cc.oracle_frames(vrt, oracle, SEED, cams, W, H, vol)
        res = cc.run_definition(W, H, cams, frames, MAX_HISTORY)
        for k in range(2):
            keep[f"{model}_camera{k}"] = np.frombuffer(bytes(cams[k]), np.uint8).copy()
            keep[f"{model}_color8_{k}"], keep[f"{model}_position_{k}"], keep[f"{model}_normal8_{k}"] = frames[k]
            for name in ("color16", "surface", "resolved8", "motion"):
                keep[f"{model}_{name}_out{k}"] = res[k][name]
        print(model, "shares of frame 1:", ref.shares(res[1]["cls"]), "wrapped", float(res[1]["wrapped"].mean()))
    np.savez_compressed(os.path.join(HERE, "render_reproject_cam.npz"), **keep)


if __name__ == "__main__":
    main()
