#!/usr/bin/env python3
"""What leaving the GPU costs (vrt_scene_list_box over every tile, vrt_scene_save_vox_mem) on the two scenes of the benchmark.

  dense   synthetic.treehouse(256, seed=2), the treehouse stand-in: one tile.  Beside the listing stands the baseline a caller had
          before it: vrt_scene_download of the whole volume plus a host-side scan for the non-zeros (np.flatnonzero), which yields
          the same voxels in the same order.
  bricks  synthetic.sparse_brick_scene(2048, 0.015, seed=5), the benchmark's brick scene (BASELINE configs[4]): 512 tiles, most of
          them over empty bricks only.  It has no baseline: vrt_scene_download refuses a brick scene, and its dense volume is 8 GiB.

Every figure is WALL time around the synchronous calls (each waits for the context's stream before it returns), median of --reps
passes, milliseconds.  No threshold is set here.  Writes profiles/export_times.json (or --out).

    python tools/exp_export.py [--reps 5] [--out profiles/export_times.json] [--skip-bricks]
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

TILE = 256


def wall_ms(fn):
    t = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t) * 1e3, r


def tiles(dims):
    for z in range(0, dims[2], TILE):
        for y in range(0, dims[1], TILE):
            for x in range(0, dims[0], TILE):
                yield (x, y, z), (min(TILE, dims[0] - x), min(TILE, dims[1] - y), min(TILE, dims[2] - z))


def list_all(scene, dims):
    n = 0
    for lo, size in tiles(dims):
        n += scene.voxels(lo, size).size
    return n


def measure(scene, dims, reps, baseline):
    row = {"dims": list(dims), "tiles": sum(1 for _ in tiles(dims))}
    tl, ts, tb = [], [], []
    for _ in range(reps):
        ms, n = wall_ms(lambda: list_all(scene, dims))
        tl.append(ms); row["voxels"] = int(n)
        ms, data = wall_ms(scene.to_vox_bytes)
        ts.append(ms); row["file_bytes"] = len(data)
        if baseline:
            def download_and_scan():
                vol, _ = scene.download()
                return np.flatnonzero(vol).size
            ms, m = wall_ms(download_and_scan)
            tb.append(ms)
            assert m == n
    row["list_tiles_ms"] = round(statistics.median(tl), 3)
    row["save_vox_mem_ms"] = round(statistics.median(ts), 3)
    if baseline:
        row["download_and_scan_ms"] = round(statistics.median(tb), 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-bricks", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "export_times.json"))
    a = ap.parse_args()
    engine = vrt.Engine(0)
    pal = vrt.synthetic.default_palette(metallic_ids=range(200, 256))
    out = {"csrc_sha16": csrc_sha16(), "device": engine.device_info(), "timing": "wall time around the synchronous calls, median of reps, milliseconds",
           "reps": a.reps, "cases": []}
    vol = vrt.synthetic.treehouse(256, seed=2)
    sc = vrt.VoxelScene.from_dense(engine, vol, pal)
    row = dict(scene="synthetic.treehouse(256, seed=2), dense", **measure(sc, (256, 256, 256), a.reps, True))
    sc.destroy()
    out["cases"].append(row); print(json.dumps(row), flush=True)
    if not a.skip_bricks:
        grid, pool = vrt.synthetic.sparse_brick_scene(2048, 0.015, seed=5)
        sc = vrt.VoxelScene.from_bricks(engine, grid, pool, pal)
        row = dict(scene="synthetic.sparse_brick_scene(2048, 0.015, seed=5), bricks", bricks=int(pool.shape[0]), **measure(sc, (2048, 2048, 2048), a.reps, False))
        sc.destroy()
        out["cases"].append(row); print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
