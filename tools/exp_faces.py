#!/usr/bin/env python3
"""What vrt_scene_list_faces costs, with and without VRT_FACES_RUNS, beside the route it replaces on the same box.

  treehouse     synthetic.treehouse(256, seed=2), the treehouse stand-in: one 256^3 tile
  checkerboard  a 256^3 checkerboard, the worst case: every solid voxel exposes six faces, no two merge (50 M records)

Per case and flag set: the whole call (count + fetch, as VoxelScene.faces makes it) and the count alone; the records; and the
route a caller had before: vrt_scene_read_box of the box plus the native single-threaded restatement of the definition
(tests/native/faces_host.cpp over csrc/vrt_faces.h), which yields the same records.  `run_ratio` is records with RUNS over records
without.  Every figure is WALL time around the synchronous calls, median of --reps passes, milliseconds.  No threshold is set here.

Per-kernel times come from a profiler, not from this script: run it once more under `rocprofv3 --kernel-trace --stats -- python
tools/exp_faces.py --reps 1 --out /dev/null` and hand the kernel statistics CSV to --kernel-stats; the k_faces_* and k_list_scan
rows are copied into the output as they stand.

    python tools/exp_faces.py [--reps 5] [--out profiles/faces_times.json] [--skip-checkerboard] [--kernel-stats FILE.csv]
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np

import voxel_raytracing_amd as vrt
from bench import csrc_sha16
import faces_native

BOX = ((0, 0, 0), (256, 256, 256))


def wall_ms(fn):
    t = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t) * 1e3, r


def measure(scene, reps, host_route):
    row = {}
    for runs in (False, True):
        name = "runs" if runs else "unit"
        tc, tf, th = [], [], []
        for _ in range(reps):
            ms, counts = wall_ms(lambda: scene.face_count(*BOX, runs=runs))
            tc.append(ms)
            ms, (rec, counts) = wall_ms(lambda: scene.faces(*BOX, runs=runs))
            tf.append(ms)
        row[name] = {"records": int(rec.size), "counts": [int(c) for c in counts], "count_ms": round(statistics.median(tc), 3),
                     "faces_ms": round(statistics.median(tf), 3)}
        if host_route:
            for _ in range(max(1, reps // 2)):
                def read_and_restate():
                    return faces_native.faces(scene.read(*BOX), (0, 0, 0), BOX[1], runs=runs)[0]
                ms, host = wall_ms(read_and_restate)
                th.append(ms)
                assert host.size == rec.size and (host == rec).all()
            row[name]["read_box_and_host_ms"] = round(statistics.median(th), 3)
    row["run_ratio"] = round(row["runs"]["records"] / max(1, row["unit"]["records"]), 4)
    return row


def kernel_rows(path):
    with open(path, newline="") as f:
        return [r for r in csv.DictReader(f) if any(k in (r.get("Name") or r.get("KernelName") or "") for k in ("k_faces_", "k_list_scan", "k_list_bricks"))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-checkerboard", action="store_true")
    ap.add_argument("--kernel-stats")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "faces_times.json"))
    a = ap.parse_args()
    engine = vrt.Engine(0)
    pal = vrt.synthetic.default_palette(metallic_ids=range(200, 256))
    out = {"csrc_sha16": csrc_sha16(), "device": engine.device_info(), "timing": "wall time around the synchronous calls, median of reps, milliseconds",
           "reps": a.reps, "cases": []}
    volumes = [("synthetic.treehouse(256, seed=2), dense", lambda: vrt.synthetic.treehouse(256, seed=2))]
    if not a.skip_checkerboard:
        z, y, x = np.meshgrid(np.arange(256), np.arange(256), np.arange(256), indexing="ij", sparse=True)
        volumes.append(("256^3 checkerboard, dense", lambda: (((x + y + z) & 1) * 9).astype(np.uint8)))
    for name, make in volumes:
        sc = vrt.VoxelScene.from_dense(engine, make(), pal)
        row = dict(scene=name, **measure(sc, a.reps, True))
        sc.destroy()
        out["cases"].append(row); print(json.dumps(row), flush=True)
    if a.kernel_stats:
        out["kernels"] = kernel_rows(a.kernel_stats)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
