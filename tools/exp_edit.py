#!/usr/bin/env python3
"""What a scene edit costs against the rebuild it replaces (vrt_scene_fill_box vs vrt_scene_free + vrt_scene_from_dense).

256^3 and 512^3 dense scenes; fills and carves of 1^3, 8^3 and 32^3 voxels in the interior and at a corner of the volume.
Every figure is WALL time around the synchronous call (both calls wait for the context's stream before they return; the
rebuild's includes the upload of the whole volume, which is what a caller without edits pays), median of --reps edits per case;
the untimed opposite edit between two timed ones restores the state.  Writes profiles/edit_times.json (or --out).

    python tools/exp_edit.py [--reps 20] [--out profiles/edit_times.json]

--bricks: the same for a brick scene made editable by vrt_scene_reserve_bricks, against vrt_scene_from_bricks of the edited
content: synthetic.sparse_brick_scene(2048, 0.015, seed=5) (BASELINE configs[4]), reserved with room for 4096 more bricks; boxes
of 1^3, 8^3 and 32^3 voxels, brick-aligned, (a) inside a block of occupied bricks -- fill: every voxel one id; carve: every voxel 0
but one per brick, so that no brick changes its occupancy -- and (b) in a block of empty bricks, where the fill creates bricks and
the carve empties them again.  After each case the scene's structures are compared with the rebuilt scene's.  Writes
profiles/brick_edit_times.json (or --out).

    python tools/exp_edit.py --bricks [--reps 20] [--out profiles/brick_edit_times.json]
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


def block_of(occ, n, want, centre):
    """low corner (z, y, x) of the n^3 block of bricks, all occupied (want) or all empty, that lies nearest to `centre`"""
    m = occ if want else ~occ
    for axis in range(3):                                         # AND over n consecutive bricks along each axis
        acc = m
        for k in range(1, n):
            acc = acc[tuple(slice(0, acc.shape[a] - 1) if a == axis else slice(None) for a in range(3))] & \
                  m[tuple(slice(k, None) if a == axis else slice(None) for a in range(3))][tuple(slice(0, acc.shape[a] - 1) if a == axis else slice(None) for a in range(3))]
        m = acc
    at = np.argwhere(m)
    if not len(at):
        raise SystemExit(f"no block of {n}^3 {'occupied' if want else 'empty'} bricks in the scene")
    return [int(v) for v in at[np.argmin(((at - (centre - n // 2)) ** 2).sum(axis=1))]]


def same_state(a, b):
    """two brick scenes' structures, canonically (the pool slot of a brick is free)"""
    K = vrt._capi
    ea, eb = a.debug_state(K.STATE_BENTRY), b.debug_state(K.STATE_BENTRY)
    ptr = np.uint64(0xFFFFFF)
    if ea.shape != eb.shape or ((ea & ~ptr) != (eb & ~ptr)).any():
        return False
    pa, pb = (ea & ptr).astype(np.int64), (eb & ptr).astype(np.int64)
    occ = (pa != 0) & (pa != 0xFFFFFF)
    if (occ != ((pb != 0) & (pb != 0xFFFFFF))).any():
        return False
    if not (np.sort(a.debug_state(K.STATE_CELLS)) == np.sort(b.debug_state(K.STATE_CELLS))).all():
        return False
    for what in (K.STATE_BPOOL, K.STATE_BFINE):
        if (a.debug_state(what)[pa[occ] - 1] != b.debug_state(what)[pb[occ] - 1]).any():
            return False
    return True


def main_bricks(a):
    engine = vrt.Engine(0)
    pal = vrt.synthetic.default_palette(metallic_ids=range(200, 256))
    N = 2048
    grid, pool = vrt.synthetic.sparse_brick_scene(N, 0.015, seed=5)
    sc = vrt.VoxelScene.from_bricks(engine, grid, pool, pal)
    sc.reserve_bricks(pool.shape[0] + 4096)
    out = {"csrc_sha16": csrc_sha16(), "device": engine.device_info(), "timing": "wall time around the synchronous call, median of reps, milliseconds",
           "scene": "synthetic.sparse_brick_scene(2048, 0.015, seed=5), reserved for 4096 more bricks", "bricks": int(pool.shape[0]),
           "memory_bytes": sc.memory_bytes(), "reps": a.reps, "cases": []}
    occ = grid != 0
    for changes, want in (("none", True), ("bricks appear / vanish", False)):
        for e in (1, 8, 32):
            nbk = max(1, e // 8)
            bz, by, bx = block_of(occ, nbk, want, N // 16)
            lo = [bx * 8, by * 8, bz * 8]
            full = np.full((e, e, e), 7, np.uint8)
            if want:                                              # one voxel per brick stays: no brick changes its occupancy
                if e == 1:
                    lo = [v + 1 for v in lo]
                    assert np.count_nonzero(pool[grid[bz, by, bx] - 1]) > 2
                carved = np.zeros((e, e, e), np.uint8)
                if e > 1:
                    carved[3::8, 3::8, 3::8] = 7
            else:
                carved = np.zeros((e, e, e), np.uint8)
            for kind, ids, other in (("fill", full, carved), ("carve", carved, full)):
                ts = []
                for _ in range(a.reps):
                    sc.edit(lo, other)                            # untimed: the opposite state
                    ts.append(wall_ms(lambda: sc.edit(lo, ids)))
                g2, p2 = vrt.synthetic.edit_bricks(grid, pool, lo, ids)

                def rebuild():
                    rebuild.scene = vrt.VoxelScene.from_bricks(engine, g2, p2, pal)
                tb = []
                for i in range(5):
                    tb.append(wall_ms(rebuild))
                    if i < 4:
                        rebuild.scene.destroy()
                ok = same_state(sc, rebuild.scene)
                rebuild.scene.destroy()
                row = {"volume": N, "occupancy_changes": changes, "box": e, "kind": kind, "lo": lo, "bricks_after": int(p2.shape[0]),
                       "edit_ms": round(statistics.median(ts), 4), "edit_ms_min": round(min(ts), 4), "edit_ms_max": round(max(ts), 4),
                       "rebuild_ms": round(statistics.median(tb), 4), "rebuild_ms_min": round(min(tb), 4), "rebuild_ms_max": round(max(tb), 4),
                       "rebuild_over_edit": round(statistics.median(tb) / statistics.median(ts), 2), "equals_rebuild": bool(ok)}
                out["cases"].append(row)
                print(json.dumps(row), flush=True)
            sc.edit(lo, np.ascontiguousarray(vrt.synthetic.dense_from_bricks(grid[bz:bz + nbk, by:by + nbk, bx:bx + nbk], pool)[
                lo[2] - bz * 8:lo[2] - bz * 8 + e, lo[1] - by * 8:lo[1] - by * 8 + e, lo[0] - bx * 8:lo[0] - bx * 8 + e]) if want else carved)   # back to the start
    sc.destroy()
    out["all_equal_rebuild"] = all(r["equals_rebuild"] for r in out["cases"])
    out["every_edit_faster"] = all(r["edit_ms"] < r["rebuild_ms"] for r in out["cases"])
    out["rebuild_over_edit_min"] = min(r["rebuild_over_edit"] for r in out["cases"])
    by_box = lambda ch, e: max(r["edit_ms"] for r in out["cases"] if r["occupancy_changes"] == ch and r["box"] == e)
    out["no_change_beats_change"] = all(by_box("none", e) < min(r["edit_ms"] for r in out["cases"] if r["occupancy_changes"] != "none" and r["box"] == e)
                                        for e in (1, 8, 32))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("equal to the rebuild:", out["all_equal_rebuild"], " every edit faster:", out["every_edit_faster"], " smallest ratio:", out["rebuild_over_edit_min"],
          " edits without a change of occupancy beat those with:", out["no_change_beats_change"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="*", default=[256, 512])
    ap.add_argument("--bricks", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "brick_edit_times.json" if a.bricks else "edit_times.json")
    if a.bricks:
        return main_bricks(a)
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
