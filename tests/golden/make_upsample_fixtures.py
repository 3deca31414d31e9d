"""Writes tests/golden/render_upsample.npz: the six 48 x 32 frames of the 48 x 32 -> 96 x 64 sequence of tests/upsample_common.py
(oracle planes and push blocks) and what the definition of temporal upsampling (tests/upsample_reference.py) makes of them --
history, resolved image and motion of every frame at 96 x 64.  It pins the DEFINITION between rounds: tests/test_upsample_cpu.py
checks that today's header and today's numpy restatement both reproduce it bit for bit.  Regenerate only on purpose:
python tests/golden/make_upsample_fixtures.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import voxel_raytracing_amd as vrt                     # host-side helpers only (synthetic scenes, camera); no GPU needed
from oracle import oracle
import reproject_common as rc
import upsample_common as uc

HERE = os.path.dirname(os.path.abspath(__file__))
PAIR, MAX_HISTORY = (48, 32, 96, 64), 32


def main():
    pushes = uc.pushes_of(vrt, oracle, PAIR)
    frames = rc.oracle_frames(vrt, oracle, uc.seed_of(PAIR), pushes)
    res = uc.run_definition(PAIR, pushes, frames, MAX_HISTORY)
    keep = {"pair": np.array(PAIR, np.int32), "frames": np.array(len(frames), np.int32), "max_history": np.array(MAX_HISTORY, np.uint32)}
    for k in range(len(frames)):
        keep[f"push{k}"] = np.frombuffer(bytes(pushes[k]), np.uint8).copy()
        keep[f"color8_{k}"], keep[f"position_{k}"], keep[f"normal8_{k}"] = frames[k]
        for name in ("color16", "surface", "resolved8", "motion"):
            keep[f"{name}_out{k}"] = res[k][name]
    print("shares:", uc.class_shares(res))
    out = os.path.join(HERE, "render_upsample.npz")
    np.savez_compressed(out, **keep)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
