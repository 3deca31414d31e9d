#!/usr/bin/env python3
"""What a scene edit costs against the rebuild it replaces (vrt_scene_fill_box vs vrt_scene_free + vrt_scene_from_dense).

256^3 and 512^3 dense scenes; fills and carves of 1^3, 8^3 and 32^3 voxels in the interior and at a corner of the volume.
Every figure is WALL time around the synchronous call (both calls wait for the context's stream before they return; the
rebuild's includes the upload of the whole volume, which is what a caller without edits pays), median of --reps edits per case;
the untimed opposite edit between two timed ones restores the state.  Writes profiles/edit_times.json (or --out).

    python tools/exp_edit.py [--reps 20] [--out profiles/edit_times.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

import voxel_raytracing_amd as vrt
from bench import csrc_sha16


def wall_ms(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="*", default=[256, 512])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edit_times.json"))
    a = ap.parse_args()
    engine = vrt.Engine(0)
    pal = vrt.synthetic.default_palette(metallic_ids=range(200, 256))
    out = {"csrc_sha16": csrc_sha16(), "device": engine.device_info(), "timing": "wall time around the synchronous call, median of reps, milliseconds",
           "reps": a.reps, "cases": []}
    for N in a.sizes:
        vol = vrt.synthetic.floating_cubes(N, seed=1, count=max(60, N))
        sc = vrt.VoxelScene.from_dense(engine, vol, pal)
        for where in ("interior", "corner"):
            for e in (1, 8, 32):
                lo = [N // 2 - e // 2] * 3 if where == "interior" else [0, 0, 0]
                for kind, vid in (("fill", 7), ("carve", 0)):
                    ts = []
                    for _ in range(a.reps):
                        sc.fill(lo, [e] * 3, 0 if vid else 7)              # untimed: the opposite state
                        ts.append(wall_ms(lambda: sc.fill(lo, [e] * 3, vid)))
                    edited = vol.copy()
                    edited[lo[2]:lo[2] + e, lo[1]:lo[1] + e, lo[0]:lo[0] + e] = vid
                    assert (sc.download()[0] == edited).all()

                    def rebuild():
                        s2 = vrt.VoxelScene.from_dense(engine, edited, pal)
                        rebuild.scene = s2
                    tb = []
                    for _ in range(5):
                        tb.append(wall_ms(rebuild))
                        rebuild.scene.destroy()
                    row = {"volume": N, "where": where, "box": e, "kind": kind, "edit_ms": round(statistics.median(ts), 4),
                           "edit_ms_min": round(min(ts), 4), "edit_ms_max": round(max(ts), 4),
                           "rebuild_ms": round(statistics.median(tb), 4), "rebuild_over_edit": round(statistics.median(tb) / statistics.median(ts), 2)}
                    out["cases"].append(row)
                    print(json.dumps(row), flush=True)
                    sc.fill(lo, [e] * 3, 0)
                    sc.edit(lo, np.ascontiguousarray(vol[lo[2]:lo[2] + e, lo[1]:lo[1] + e, lo[0]:lo[0] + e]))     # back to the start
        sc.destroy()
    out["every_edit_faster"] = all(r["edit_ms"] < r["rebuild_ms"] for r in out["cases"])
    out["rebuild_over_edit_min"] = min(r["rebuild_over_edit"] for r in out["cases"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("every edit faster than the rebuild:", out["every_edit_faster"], " smallest ratio:", out["rebuild_over_edit_min"])


if __name__ == "__main__":
    main()
