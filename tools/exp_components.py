#!/usr/bin/env python3
"""What labelling every component of 512^3 bounds costs (vrt_scene_components), what a despeckle costs on top
(vrt_scene_filter_components), and, for comparison, what the library offered for the same question before: one
vrt_scene_flood under VRT_FLOOD_MEASURE from the root of the largest component of the same bounds.

Scenes: the benchmark's stand-in scene (synthetic.treehouse) and synthetic.mandelbulb at 512^3, each dense and as bricks (reserved,
so that the despeckle can write).  Per scene, SOLID under 6-connectivity: the labelling, a despeckle below --speck voxels (the
scene is restored after it), and the measuring flood, in turn in the same process.  Every figure is WALL time around the
synchronous calls, median of --reps.  Nothing is gated on these numbers.  Writes profiles/components_times.json; the per-kernel
split comes from a kernel trace of this script (tools/trace_any.sh), the kernels' resources from
profiles/components_kernel_digest.txt.

    python tools/exp_components.py [--reps 5] [--size 512] [--speck 8] [--out profiles/components_times.json]
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
    out = fn()
    return (time.perf_counter() - t) * 1e3, out


def case(engine, name, vol, bricks, reps, speck):
    pal = vrt.synthetic.default_palette(metallic_ids=range(200, 256))
    n = vol.shape[0]
    if bricks:
        grid, pool = vrt.synthetic.bricks_from_dense(vol)
        sc = vrt.VoxelScene.from_bricks(engine, grid, pool, pal)
        sc.reserve_bricks(pool.shape[0] + 64)
    else:
        sc = vrt.VoxelScene.from_dense(engine, vol, pal)
    label, filt, flood = [], [], []
    rec = res = got = None
    for _ in range(reps):
        ms, (rec, res) = wall_ms(lambda: sc.components("solid", 6))
        label.append(ms)
        root = tuple(int(v) for v in rec[res["largest"]]["root"]) if res["components"] else (0, 0, 0)
        ms, region = wall_ms(lambda: sc.region(root, "solid", 6))
        flood.append(ms)
        assert not res["components"] or region[0] == int(rec[res["largest"]]["voxels"]), (region, rec[res["largest"]])
        ms, got = wall_ms(lambda: sc.despeckle(speck))
        filt.append(ms)
        if got["changed"]:                                        # put the specks back
            lo, size = got["lo"], got["size"]
            sc.edit(lo, np.ascontiguousarray(vol[lo[2]:lo[2] + size[2], lo[1]:lo[1] + size[1], lo[0]:lo[0] + size[0]]))
    row = {"case": name, "bricks": bricks, "size": n, "components": res["components"], "voxels": res["voxels"],
           "largest_voxels": int(rec[res["largest"]]["voxels"]) if res["components"] else 0, "flood_rounds": sc.flood_rounds(),
           "label_ms": statistics.median(label), "label_ms_all": label, "despeckle_ms": statistics.median(filt), "despeckle_changed": got["changed"],
           "flood_measure_ms": statistics.median(flood)}
    row["label_over_flood"] = row["label_ms"] / row["flood_measure_ms"]
    print(json.dumps(row), flush=True)
    sc.destroy()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--speck", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "components_times.json"))
    a = ap.parse_args()
    engine = vrt.Engine(0)
    rows = []
    for name, vol in (("treehouse", vrt.synthetic.treehouse(a.size, seed=2)), ("mandelbulb", vrt.synthetic.mandelbulb(a.size))):
        for bricks in (False, True):
            rows.append(case(engine, f"{name} {a.size}^3, {'bricks' if bricks else 'dense'}", vol, bricks, a.reps, a.speck))
    with open(a.out, "w") as f:
        json.dump({"commit_csrc_sha16": csrc_sha16(), "device": engine.device_info(), "reps": a.reps, "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
