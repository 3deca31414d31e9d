#!/usr/bin/env python3
"""What a flood on the device costs against the round trip it replaces (vrt_scene_flood vs vrt_scene_read_box -> a flood on the
host -> vrt_scene_edit_box).

Selections: the air of a 256^3 and a 512^3 box of the benchmark's stand-in scene (synthetic.treehouse) under VRT_FLOOD_MEASURE,
one object's recolour in the 256^3 scene, and the serpentine of tests/flood_common.py.  Every figure is WALL time around the
synchronous calls, median of --reps; the device figures come with the number of rounds the tile kernel ran.  The host's flood is
scipy.ndimage.label where scipy is installed, else a numpy loop of dilations (and then left out at 512^3, where it takes minutes):
the round trip's read and edit are timed either way.  Nothing is gated on these numbers.  Writes profiles/flood_times.json.

    python tools/exp_flood.py [--reps 5] [--out profiles/flood_times.json]
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


def wall_ms(fn):
    t = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t) * 1e3, out


def host_component(passable, seed, big):
    """the 6-connected component of seed (x, y, z) in a bool volume [z, y, x], or None where that would take minutes"""
    try:
        from scipy import ndimage
        lab, _ = ndimage.label(passable)
        return lab == lab[seed[2], seed[1], seed[0]]
    except ImportError:
        if big:
            return None
    reach = np.zeros_like(passable)
    reach[seed[2], seed[1], seed[0]] = passable[seed[2], seed[1], seed[0]]
    while True:
        grow = reach.copy()
        for axis in range(3):
            lo = [slice(None)] * 3; hi = [slice(None)] * 3
            lo[axis], hi[axis] = slice(0, -1), slice(1, None)
            grow[tuple(hi)] |= reach[tuple(lo)]; grow[tuple(lo)] |= reach[tuple(hi)]
        grow &= passable
        if (grow == reach).all():
            return reach
        reach = grow


def case(sc, vol, name, seed, vid, match, measure, reps, restore):
    dims = (vol.shape[2], vol.shape[1], vol.shape[0])
    dev, trip, rounds, region = [], [], 0, 0
    for _ in range(reps):
        if measure:
            ms, got = wall_ms(lambda: sc.region(seed, match))
            region = got[0]
        else:
            ms, got = wall_ms(lambda: sc.flood(seed, vid, match))
            region = got["region"]
            restore()
        dev.append(ms); rounds = sc.flood_rounds()
    host = {"read_ms": [], "flood_ms": [], "edit_ms": []}
    for _ in range(max(1, reps // 2)):
        ms, box = wall_ms(lambda: sc.read((0, 0, 0), dims))
        host["read_ms"].append(ms)
        sid = box[seed[2], seed[1], seed[0]]
        ms, reg = wall_ms(lambda: host_component((box == sid) if match == "same" else (box != 0), seed, vol.size > 1 << 25))
        if reg is not None:
            host["flood_ms"].append(ms)
            assert int(reg.sum()) == region, (name, int(reg.sum()), region)
        if not measure:
            new = box.copy()
            if reg is not None:
                new[reg] = vid
            ms, _ = wall_ms(lambda: sc.edit((0, 0, 0), new))
            host["edit_ms"].append(ms)
            restore()
    row = {"case": name, "dims": list(dims), "seed": list(seed), "match": match, "measure": measure, "region": region, "rounds": rounds,
           "device_ms": statistics.median(dev), "device_ms_all": dev}
    for k, v in host.items():
        row["host_" + k] = statistics.median(v) if v else None
    parts = [row["host_read_ms"], row["host_flood_ms"]] + ([row["host_edit_ms"]] if not measure else [])
    row["round_trip_ms"] = sum(parts) if all(p is not None for p in parts) else None
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flood_times.json"))
    ap.add_argument("--sizes", default="256,512")
    a = ap.parse_args()
    import flood_common as fc
    engine = vrt.Engine(0)
    pal = vrt.synthetic.default_palette(metallic_ids=range(200, 256))
    rows = []
    for n in [int(t) for t in a.sizes.split(",")]:
        vol = vrt.synthetic.treehouse(n, seed=2)
        sc = vrt.VoxelScene.from_dense(engine, vol, pal)
        air = tuple(int(v) for v in np.argwhere(vol == 0)[0][::-1])
        rows.append(case(sc, vol, f"air of the {n}^3 stand-in scene", air, 0, "same", True, a.reps, lambda: None))
        if n == 256:
            solid = tuple(int(v) for v in np.argwhere(vol != 0)[len(np.argwhere(vol != 0)) // 2][::-1])
            rows.append(case(sc, vol, "recolour of one object (same id, 6)", solid, 250, "same", False, a.reps, lambda: sc.edit((0, 0, 0), vol)))
        sc.destroy()
    vol, first, _, path = fc.serpentine_volume()
    sc = vrt.VoxelScene.from_dense(engine, vol, pal)
    rows.append(case(sc, vol, "serpentine 24x24x8", first, 2, "same", False, a.reps, lambda: sc.edit((0, 0, 0), vol)))
    sc.destroy()
    with open(a.out, "w") as f:
        json.dump({"commit_csrc_sha16": csrc_sha16(), "device": engine.device_info(), "reps": a.reps, "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
