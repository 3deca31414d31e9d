#!/usr/bin/env python3
"""What a brush costs against the route it replaces (vrt_scene_brush vs read the bounding box, compose in numpy, edit the box).

256^3 and 512^3 dense scenes (synthetic.floating_cubes) and the benchmark's brick scene (synthetic.sparse_brick_scene(2048,
0.015, seed=5), reserved for 4096 more bricks); spheres of radius 1, 4, 16 and 64 voxels in SET, PAINT and ADD at the centre of the
volume, and a PAINT over air (a no-op).  Every figure is WALL time around the synchronous calls, median of --reps; the host route
uses only VoxelScene.read, numpy and VoxelScene.edit.  Between two timed runs the bounding box is put back with an untimed edit, so
every run starts from the same scene, and after the first run of each case both routes' volumes are compared.  kernel_share: the
two new kernels' time (hipEvents around them would need a hook in the library; here: the brush's wall time minus the wall time of
vrt_scene_edit_box of the returned tight box with the same ids, clamped at 0) over the brush's.  Writes profiles/brush_times.json.

    python tools/exp_brush.py [--reps 20] [--out profiles/brush_times.json] [--sizes 256 512] [--no-bricks]
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


def sphere_mask(n, r2):
    """bool [z, y, x] of the n^3 box around a sphere centred on the box's middle corner: |d|^2 <= r2 in half voxels"""
    d = (2 * np.arange(n) + 1 - n).astype(np.int64)
    return (d[:, None, None] ** 2 + d[None, :, None] ** 2 + d[None, None, :] ** 2) <= r2


def compose(old, mask, mode, vid):
    if mode == "set":
        return np.where(mask, np.uint8(vid), old)
    if mode == "paint":
        return np.where(mask & (old != 0), np.uint8(vid), old)
    return np.where(mask & (old == 0), np.uint8(vid), old)


def run_cases(sc, N, label, reps, rows, air_centre, radii=(1, 4, 16, 64)):
    c = N // 2
    cases = [(r, m, (c, c, c)) for r in radii for m in ("set", "paint", "add")] + [(3, "paint-over-air", air_centre)]
    for r, mode, centre in cases:
        m = "paint" if mode == "paint-over-air" else mode
        lo, n = [v - r for v in centre], 2 * r
        mask = sphere_mask(n, (2 * r) ** 2)
        start = sc.read(lo, [n] * 3)
        tb, th, te = [], [], []
        res = None
        for k in range(reps):
            res = [None]
            tb.append(wall_ms(lambda: res.__setitem__(0, sc.sphere(centre, r, 77, m))))
            after_brush = sc.read(lo, [n] * 3) if k == 0 else None
            if res[0][0] and k < 5:                            # the tight box alone, ids from the host: what the edit passes cost
                tl, ts = res[0][1], res[0][2]
                ids = sc.read(tl, ts)
                sc.edit(lo, start)
                te.append(wall_ms(lambda: sc.edit(tl, ids)))
            sc.edit(lo, start)                                 # untimed: back to the start

            def host_route():
                old = sc.read(lo, [n] * 3)
                sc.edit(lo, compose(old, mask, m, 77))
            th.append(wall_ms(host_route))
            if k == 0:
                assert (sc.read(lo, [n] * 3) == after_brush).all(), (label, r, mode)
            sc.edit(lo, start)
        brush, host = statistics.median(tb), statistics.median(th)
        edit = statistics.median(te) if te else 0.0
        row = {"scene": label, "radius": r, "mode": mode, "changed": int(res[0][0]), "tight_box": list(res[0][2]), "bounding_box": n,
               "brush_ms": round(brush, 4), "brush_ms_min": round(min(tb), 4), "brush_ms_max": round(max(tb), 4),
               "host_route_ms": round(host, 4), "host_route_ms_min": round(min(th), 4), "host_route_ms_max": round(max(th), 4),
               "host_over_brush": round(host / brush, 2), "tight_edit_ms": round(edit, 4),
               "kernel_share": round(max(0.0, brush - edit) / brush, 3) if te else 1.0}
        rows.append(row)
        print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="*", default=[256, 512])
    ap.add_argument("--no-bricks", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "brush_times.json"))
    a = ap.parse_args()
    engine = vrt.Engine(0)
    pal = vrt.synthetic.default_palette(metallic_ids=range(200, 256))
    out = {"csrc_sha16": csrc_sha16(), "device": engine.device_info(), "timing": "wall time around the synchronous calls, median of reps, milliseconds",
           "host_route": "VoxelScene.read of the bounding box, numpy compose, VoxelScene.edit of the bounding box", "reps": a.reps, "cases": []}
    for N in a.sizes:
        vol = vrt.synthetic.floating_cubes(N, seed=1, count=max(60, N))
        vol[N // 2 - 70:N // 2 + 70, N // 2 - 70:N // 2 + 70, N // 2 - 70:N // 2 + 70:2] = 5      # something to paint and something to add to
        vol[8:48, 8:48, 8:48] = 0                                                                # air for the no-op
        sc = vrt.VoxelScene.from_dense(engine, vol, pal)
        run_cases(sc, N, "dense %d^3" % N, a.reps, out["cases"], (28, 28, 28))
        sc.destroy()
    if not a.no_bricks:
        N = 2048
        grid, pool = vrt.synthetic.sparse_brick_scene(N, 0.015, seed=5)
        empty = np.argwhere(grid[2:-2, 2:-2, 2:-2] == 0)[0] + 2
        sc = vrt.VoxelScene.from_bricks(engine, grid, pool, pal)
        sc.reserve_bricks(pool.shape[0] + 4096)
        # (radius 64 left out: a SET or ADD of that size wants about 2 500 slots at once, more than the centre's neighbourhood leaves of the 4096)
        run_cases(sc, N, "bricks 2048^3", a.reps, out["cases"], tuple(int(v) * 8 + 4 for v in empty[::-1]), radii=(1, 4, 16))
        sc.destroy()
    out["every_brush_faster"] = all(r["brush_ms"] < r["host_route_ms"] for r in out["cases"])
    out["host_over_brush_min"] = min(r["host_over_brush"] for r in out["cases"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("every brush faster than the host route:", out["every_brush_faster"], " smallest ratio:", out["host_over_brush_min"])


if __name__ == "__main__":
    main()
