#!/usr/bin/env python3
"""What morphology on the device costs against the round trip it replaces (vrt_scene_morph vs vrt_scene_read_box -> the native
restatement of csrc/vrt_morph.h on one CPU thread, tests/native/morph_host.cpp -> vrt_scene_edit_box).

Scenes: a 256^3 box of the benchmark's stand-in scene (synthetic.treehouse), dense, whole-volume bounds; and the benchmark's brick
scene (synthetic.sparse_brick_scene(2048, 0.015, seed=5); --brick-size) inside 512^3 bounds at its centre.  Per operation at r = 1 and r = 8 (connectivity 6): the whole call, the
call under VRT_MORPH_MEASURE (the mask pass, the phases and the extent kernel without the edit passes; the difference is the edit
behind the compose kernel), and the host route, interleaved with the device calls in the same process; the scene is restored
after every call that writes.  Every figure is WALL time around the synchronous calls, median of --reps.  Nothing is gated on
these numbers: a size at which the device route is not faster is reported like any other.  Writes profiles/morph_times.json.

    python tools/exp_morph.py [--reps 5] [--brick-size 2048] [--out profiles/morph_times.json]
"""
import argparse
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

OPS = ("dilate", "erode", "open", "close", "hollow")


def wall_ms(fn):
    t = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t) * 1e3, out


def case(sc, name, op, r, lo, size, reps):
    import morph_native as N
    import morph_reference as M
    vid = 250 if op in ("dilate", "close") else 0
    bounds = (lo, size)
    old = sc.read(lo, size)
    dev, meas, host = [], [], {"read_ms": [], "morph_ms": [], "edit_ms": []}
    res = None
    for _ in range(reps):                                          # device and host route in turn
        ms, got = wall_ms(lambda: sc.morph(op, r, 6, vid, bounds, measure=True))
        meas.append(ms)
        ms, res = wall_ms(lambda: sc.morph(op, r, 6, vid, bounds))
        dev.append(ms)
        assert (res["added"], res["removed"]) == (got["added"], got["removed"])
        sc.edit(lo, old)
        # the host route reads the bounds and their halo, as far as the volume goes
        h = M.halo(M.OPS[op], r)
        dims = (sc.width, sc.height, sc.depth)
        hlo = [max(0, lo[a] - h) for a in range(3)]
        hsz = [min(dims[a], lo[a] + size[a] + h) - hlo[a] for a in range(3)]
        ms, box = wall_ms(lambda: sc.read(hlo, hsz))
        host["read_ms"].append(ms)
        inner = ([lo[a] - hlo[a] for a in range(3)], list(size))
        ms, (rc, new, hres) = wall_ms(lambda: N.morph(box, M.OPS[op], r, 6, vid, inner))
        host["morph_ms"].append(ms)
        exact = all(hlo[a] == lo[a] - h or hlo[a] == 0 for a in range(3)) and all(hlo[a] + hsz[a] in (lo[a] + size[a] + h, dims[a]) for a in range(3))
        assert rc == 0 and (not exact or (hres["added"], hres["removed"]) == (res["added"], res["removed"])), (name, op, r, hres, res)
        i = inner[0]
        ms, _ = wall_ms(lambda: sc.edit(lo, np.ascontiguousarray(new[i[2]:i[2] + size[2], i[1]:i[1] + size[1], i[0]:i[0] + size[0]])))
        host["edit_ms"].append(ms)
        sc.edit(lo, old)
    row = {"case": name, "op": op, "radius": r, "lo": list(lo), "size": list(size), "added": res["added"], "removed": res["removed"],
           "device_ms": statistics.median(dev), "device_ms_all": dev, "measure_ms": statistics.median(meas)}
    for k, v in host.items():
        row["host_" + k] = statistics.median(v)
    row["round_trip_ms"] = row["host_read_ms"] + row["host_morph_ms"] + row["host_edit_ms"]
    row["device_faster"] = row["device_ms"] < row["round_trip_ms"]
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--brick-size", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "morph_times.json"))
    a = ap.parse_args()
    engine = vrt.Engine(0)
    pal = vrt.synthetic.default_palette(metallic_ids=range(200, 256))
    rows = []
    vol = vrt.synthetic.treehouse(256, seed=2)
    sc = vrt.VoxelScene.from_dense(engine, vol, pal)
    for op in OPS:
        for r in (1, 8):
            rows.append(case(sc, "dense 256^3, whole volume", op, r, (0, 0, 0), (256, 256, 256), a.reps))
    sc.destroy()
    n = a.brick_size
    grid, pool = vrt.synthetic.sparse_brick_scene(n, 0.015, seed=5)
    sc = vrt.VoxelScene.from_bricks(engine, grid, pool, pal)
    sc.reserve_bricks(pool.shape[0] + 64 ** 3)                        # a dilation of the bounds can occupy every brick in and around them
    lo = tuple((n - 512) // 2 for _ in range(3))
    for op in OPS:
        for r in (1, 8):
            rows.append(case(sc, f"bricks {n}^3, bounds 512^3", op, r, lo, (512, 512, 512), a.reps))
    sc.destroy()
    with open(a.out, "w") as f:
        json.dump({"commit_csrc_sha16": csrc_sha16(), "device": engine.device_info(), "reps": a.reps, "rows": rows,
                   "every_case_faster": all(r["device_faster"] for r in rows)}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
