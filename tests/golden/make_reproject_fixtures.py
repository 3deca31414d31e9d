"""Writes tests/golden/render_reproject.npz: two 32 x 24 frames of the moving sequence of tests/reproject_common.py (oracle
planes and push blocks) and what the definition of temporal reprojection (tests/reproject_reference.py) makes of them -- history,
resolved image and motion of both frames.  It pins the DEFINITION between rounds: tests/test_reproject_cpu.py checks that today's
header and today's numpy restatement both reproduce it bit for bit.  Regenerate only on purpose:
python tests/golden/make_reproject_fixtures.py"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import voxel_raytracing_amd as vrt                     # host-side helpers only (synthetic scenes, camera); no GPU needed
from oracle import oracle
import reproject_common as rc
import reproject_reference as ref

HERE = os.path.dirname(os.path.abspath(__file__))
W, H, SEED, MAX_HISTORY = 32, 24, 1, 32


def main():
    pushes = rc.pushes_of(vrt, oracle, W, H, frames=2)
    frames = rc.oracle_frames(vrt, oracle, SEED, pushes)
    res = rc.run_definition(W, H, pushes, frames, MAX_HISTORY)
    keep = {"max_history": np.array(MAX_HISTORY, np.uint32)}
    for k in range(2):
        keep[f"push{k}"] = np.frombuffer(bytes(pushes[k]), np.uint8).copy()
        keep[f"color8_{k}"], keep[f"position_{k}"], keep[f"normal8_{k}"] = frames[k]
        for name in ("color16", "surface", "resolved8", "motion"):
            keep[f"{name}_out{k}"] = res[k][name]
    print("shares of frame 1:", ref.shares(res[1]["cls"]))
    np.savez_compressed(os.path.join(HERE, "render_reproject.npz"), **keep)


if __name__ == "__main__":
    main()
