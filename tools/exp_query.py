#!/usr/bin/env python3
"""What ray queries cost, and what an incoherent ray order costs (vrt_pick_pixels, vrt_trace_rays, vrt_occluded_rays).

The bench scene (treehouse stand-in, 256^3, default camera, 1920 x 1080) and the 2048^3 brick scene of the brick tools
(synthetic.sparse_brick_scene(2048, 0.015, seed=5)), every pixel of the frame one ray:
  (a) vrt_pick_pixels, pixels in 8x8-block order (a wave's 64 rays are K1's 8x8 block)      (b) the same, row-major
  (c) vrt_trace_rays of the same rays from buffers, in both orders                             (d) under a fixed random permutation
  (e) vrt_occluded_rays of (c)
  (f) the yardstick, dense scene only: primary_ms of a primary-only vrt_render_geometry of that frame (the reference's six
      targets), with tile_tags and sky_fast on and with both off
Times are HIP events on the engine's stream around one call, after --warmup calls, the median of --reps (>= 20).  Writes
profiles/ray_query_times.json (or --out): times, rays per second, ratios to the yardstick, the digest of the library's sources,
the device name; and whether (a) in block order costs more than the yardstick without tags and sky path plus the time to
stream the query's extra bytes (the xy plane it reads, 8 B per ray, and its voxel plane being 6 B per ray wider than
hit_voxel) at the HBM rate DESIGN.md 7 uses, 8 TB/s -- the case DESIGN.md has to explain.

    python tools/exp_query.py [--reps 20] [--warmup 3] [--no-bricks] [--out profiles/ray_query_times.json]

--segments measures the queries with a distance limit instead (vrt_trace_segments, vrt_occluded_segments; measure_segments says
what) on the same scenes, frame and ray orders, and writes profiles/segment_times.json.
"""
import argparse
import hashlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

import voxel_raytracing_amd as vrt
from bench import csrc_sha16

HBM_BYTES_PER_S = 8e12
W, H = 1920, 1080


def query_sha16():
    h = hashlib.sha256()
    for n in ("vrt_query.hip", "vrt_query.h", "vrt_device_common.h"):
        with open(os.path.join(ROOT, "voxel-raytracing_amd", "csrc", n), "rb") as f:
            h.update(n.encode() + b"\0" + f.read())
    return h.hexdigest()[:16]


def event_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times), "reps": reps}


def pixel_orders():
    ys, xs = np.mgrid[0:H, 0:W]
    row = np.stack([xs.reshape(-1), ys.reshape(-1)], axis=1).astype(np.int32)
    # 8x8 blocks, row-major over the blocks, row-major within (lane l -> (l & 7, l >> 3): K1's wave)
    by, bx, ly, lx = np.meshgrid(np.arange(H // 8), np.arange(W // 8), np.arange(8), np.arange(8), indexing="ij")
    block = np.stack([(bx * 8 + lx).reshape(-1), (by * 8 + ly).reshape(-1)], axis=1).astype(np.int32)
    assert len(block) == W * H
    return {"block8x8": block, "row_major": row}


def primary_rays(push, xy):
    """main()'s rays (voxel_volume.frag:312-322) in numpy float32: the timing needs the frame's rays, not their last bit"""
    f = np.float32
    Wf, Hf = f(push.screen_size[0]), f(push.screen_size[1])
    sx = ((xy[:, 0].astype(f) + f(0.5)) / Wf) * f(2) - f(1)
    sy = ((xy[:, 1].astype(f) + f(0.5)) / Hf) * f(2) - f(1)
    cd = np.array(list(push.cam_dir)[:3], f); cd = cd / np.sqrt((cd * cd).sum(dtype=f))
    U = np.array(list(push.cam_right)[:3], f); V = np.array(list(push.cam_up)[:3], f) * Hf / Wf
    jit = np.array([push.camera_jitter[0] / Wf * f(-2), push.camera_jitter[1] / Hf * f(2), 0], f)
    v = cd[None, :] + sx[:, None] * U[None, :] + sy[:, None] * V[None, :] + jit[None, :]
    d = (v / np.sqrt((v * v).sum(axis=1, dtype=f))[:, None]).astype(f)
    o = np.broadcast_to(np.array(list(push.cam_pos)[:3], f), d.shape).copy()
    return o, d


def measure_scene(engine, scene, push, a, orders):
    dev = engine.torch_device
    n = W * H
    out = {}
    xy_dev = {k: torch.from_numpy(v).to(dev) for k, v in orders.items()}
    rec = None
    for k, t in xy_dev.items():
        out[f"pick_{k}"] = event_ms(lambda: scene.pick(push, t, 512), a.warmup, a.reps)
        rec = scene.pick(push, t, 512)
    out["hit_fraction"] = float((rec["material"] != 0).float().mean().item())
    perm = np.random.default_rng(1).permutation(n)
    ray_sets = dict(orders)
    ray_sets["random_permutation"] = orders["row_major"][perm]
    for k, xy in ray_sets.items():
        o, d = primary_rays(push, xy)
        o, d = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
        out[f"trace_{k}"] = event_ms(lambda: scene.trace_rays(o, d, 512), a.warmup, a.reps)
        out[f"occluded_{k}"] = event_ms(lambda: scene.occluded(o, d, 512), a.warmup, a.reps)
    for k, v in out.items():
        if isinstance(v, dict):
            v["rays_per_s"] = n / (v["median_ms"] * 1e-3)
    return out


def yardstick(engine, scene, push, a):
    st = vrt.VoxelRenderSettings.primary_only((W, H))
    stage = vrt.GeometryStage(engine, st, scene)
    res = {}
    for name, opts in (("tags_and_sky_fast_on", {"tile_tags": 1, "sky_fast": 1}), ("tags_and_sky_fast_off", {"tile_tags": 0, "sky_fast": 0})):
        with engine.options(**opts):
            for _ in range(a.warmup):
                stage.record(push)
            engine.synchronize()
            times = []
            for _ in range(a.reps):
                stage.record(push)
                times.append(engine.last_timings()["primary_ms"])
        res[name] = {"median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times), "reps": a.reps}
    return res


def wall_ms(fn, warmup, reps):
    """Wall-clock time of a call that ends with its result on the host (it synchronises itself)."""
    import time
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter(); fn(); times.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times), "reps": reps}


ROUNDS = 5


def alternating(cases, engine, a):
    """cases: {name: (segment_budget or None, fn)}.  ROUNDS rounds; in each, every case is timed once (a.warmup calls, then a.reps
    between HIP events), in the given order in even rounds and reversed in odd ones.  Per case: the median of every round, their
    median (median_ms), their smallest and largest (the run-to-run spread of a median), and the extremes of all single calls."""
    names = list(cases)
    per = {k: [] for k in names}
    for rnd in range(ROUNDS):
        for k in (names if rnd % 2 == 0 else names[::-1]):
            budget, fn = cases[k]
            if budget is None:
                per[k].append(event_ms(fn, a.warmup, a.reps))
            else:
                with engine.options(segment_budget=budget):
                    per[k].append(event_ms(fn, a.warmup, a.reps))
    out = {}
    for k, rs in per.items():
        meds = [x["median_ms"] for x in rs]
        out[k] = {"median_ms": statistics.median(meds), "round_medians_ms": meds, "median_lo_ms": min(meds), "median_hi_ms": max(meds),
                  "min_ms": min(x["min_ms"] for x in rs), "max_ms": max(x["max_ms"] for x in rs), "reps": a.reps, "rounds": ROUNDS}
    return out


def measure_segments(engine, scene, push, dims, a, orders):
    """--segments, one scene.  Rays: the frame's primary rays in 8x8-block order (coherent) and under a fixed random permutation
    (shuffled), as they leave the camera and once more moved to where they enter the volume ("from_entry": a segment then starts
    at the volume's face, as a shadow ray or a line of sight inside a level does).  Unit directions: t is in voxels.
      1  vrt_trace_segments with t_max = +inf against vrt_trace_rays (the parent's kernel) on the same rays
      2  vrt_occluded_segments with t_max = 1/16, 1/4, 1 of the volume's diagonal and +inf, segment_budget 1 and 0 in turn (alternating)
      3  line of sight over 1/4 of the diagonal: VoxelScene.visible against vrt_trace_rays + pos copied to the host + a numpy compare"""
    dev = engine.torch_device
    n = W * H
    diag = float(np.sqrt(sum(float(x) ** 2 for x in dims)))
    perm = np.random.default_rng(1).permutation(n)
    xy_sets = {"coherent": orders["block8x8"], "shuffled": orders["row_major"][perm]}
    out = {"diagonal_voxels": diag}
    for order, xy in xy_sets.items():
        o, d = primary_rays(push, xy)
        with np.errstate(divide="ignore", invalid="ignore"):
            size = np.array(dims, np.float32)
            t1, t2 = (-o) / d, (size[None, :] - o) / d
            tmin = np.fmax.reduce(np.fmin(t1, t2), axis=1); tmax = np.fmin.reduce(np.fmax(t1, t2), axis=1)
        enters = (tmax >= np.maximum(tmin, 0))
        o_in = np.where(enters[:, None], o + np.maximum(tmin, 0)[:, None] * d, o).astype(np.float32)
        for origin, oo in (("from_camera", o), ("from_entry", o_in)):
            key = f"{order}_{origin}"
            to, td = torch.from_numpy(oo).to(dev), torch.from_numpy(d).to(dev)
            inf = torch.full((n,), float("inf"), dtype=torch.float32, device=dev)
            limits = {"inf": inf}
            for frac, label in ((1.0 / 16, "diag_16th"), (0.25, "diag_quarter"), (1.0, "diag")):
                limits[label] = torch.full((n,), diag * frac, dtype=torch.float32, device=dev)
            # every case of a group in turn, ROUNDS times over, the order reversed every other round: what is compared is timed
            # side by side, and the ROUNDS medians of one case are its run-to-run spread
            r = alternating({"trace_rays": (None, lambda: scene.trace_rays(to, td, 512)),
                             "trace_segments_inf_budget1": (1, lambda: scene.trace_segments(to, td, inf, 512)),
                             "trace_segments_inf_budget0": (0, lambda: scene.trace_segments(to, td, inf, 512))}, engine, a)
            for label, tm in limits.items():
                group = {f"occluded_segments_{label}_budget1": (1, lambda tm=tm: scene.occluded(to, td, 512, t_max=tm)),
                         f"occluded_segments_{label}_budget0": (0, lambda tm=tm: scene.occluded(to, td, 512, t_max=tm))}
                if label == "inf":
                    group["occluded_rays"] = (None, lambda: scene.occluded(to, td, 512))
                r.update(alternating(group, engine, a))
                if label != "inf":
                    r[f"occluded_fraction_{label}"] = float(scene.occluded(to, td, 512, t_max=tm).float().mean().item())
            r["ratio_trace_segments_inf_to_trace_rays"] = r["trace_segments_inf_budget1"]["median_ms"] / r["trace_rays"]["median_ms"]
            out[key] = r
        # 3: the caller's alternative, host arrays in and out on both sides
        L = np.float32(0.25 * diag)
        a_pts, b_pts = o_in, (o_in + L * d).astype(np.float32)

        def alternative():
            rec = scene.trace_rays(a_pts, b_pts - a_pts, 512, planes=("material", "pos"))
            dist = np.linalg.norm(rec["pos"] - a_pts, axis=1)
            return ~((rec["material"] != 0) & (dist <= np.linalg.norm(b_pts - a_pts, axis=1)))

        out[f"{order}_line_of_sight"] = {"visible": wall_ms(lambda: scene.visible(a_pts, b_pts, 512), a.warmup, a.reps),
                                         "trace_rays_pos_to_host_numpy": wall_ms(alternative, a.warmup, a.reps),
                                         "disagreements": int((scene.visible(a_pts, b_pts, 512) != alternative()).sum()),
                                         "note": "wall clock, uploads and downloads included on both sides; the alternative compares rounded distances, so a few pairs at the limit may differ"}
    return out


def main_segments(a):
    engine = vrt.Engine(0)
    name, cus = engine.device_info()
    pal = vrt.synthetic.default_palette(metallic_ids=range(200, 256))
    orders = pixel_orders()
    result = {"tool": "tools/exp_query.py --segments", "device": name, "compute_units": cus, "csrc_sha16": csrc_sha16(), "frame": [W, H], "rays": W * H,
              "max_steps": 512, "timing": "HIP events on the engine's stream around one call after --warmup calls, --reps calls per round; the cases that are compared alternate over 5 rounds: "
                        "median_ms is the median of the rounds' medians, median_lo / median_hi their range (the run-to-run spread), min / max the extremes of single calls; line of sight: wall clock",
              "warmup": a.warmup, "scenes": {}}
    N = 256
    scene = vrt.VoxelScene.from_dense(engine, vrt.synthetic.treehouse(N, seed=2), pal)
    pos, yaw, pitch = vrt.synthetic.default_camera_for(N, N, N)
    push = vrt.make_push(vrt.CameraController(position=pos, yaw=yaw, pitch=pitch), (N, N, N), (W, H))
    result["scenes"]["treehouse_256"] = measure_segments(engine, scene, push, (N, N, N), a, orders)
    scene.destroy()
    if not a.no_bricks:
        N = 2048
        grid, pool = vrt.synthetic.sparse_brick_scene(N, 0.015, seed=5)
        scene = vrt.VoxelScene.from_bricks(engine, grid, pool, pal)
        pos, yaw, pitch = vrt.synthetic.default_camera_for(N, N, N)
        push = vrt.make_push(vrt.CameraController(position=pos, yaw=yaw, pitch=pitch), (N, N, N), (W, H))
        result["scenes"]["sparse_bricks_2048"] = measure_segments(engine, scene, push, (N, N, N), a, orders)
        scene.destroy()
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-bricks", action="store_true")
    ap.add_argument("--segments", action="store_true", help="measure vrt_trace_segments / vrt_occluded_segments instead (profiles/segment_times.json)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit("--reps: at least 20")
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "segment_times.json" if a.segments else "ray_query_times.json")
    if a.segments:
        return main_segments(a)
    engine = vrt.Engine(0)
    name, cus = engine.device_info()
    pal = vrt.synthetic.default_palette(metallic_ids=range(200, 256))
    orders = pixel_orders()
    result = {"tool": "tools/exp_query.py", "device": name, "compute_units": cus, "csrc_sha16": csrc_sha16(), "query_sha16": query_sha16(),
              "frame": [W, H], "rays": W * H, "max_steps": 512, "timing": "HIP events on the engine's stream around one call, median", "scenes": {}}

    N = 256
    scene = vrt.VoxelScene.from_dense(engine, vrt.synthetic.treehouse(N, seed=2), pal, sky=vrt.synthetic.sky_gradient(512, 256),
                                      noise=vrt.synthetic.blue_noise_standin(512))
    pos, yaw, pitch = vrt.synthetic.default_camera_for(N, N, N)
    push = vrt.make_push(vrt.CameraController(position=pos, yaw=yaw, pitch=pitch), (N, N, N), (W, H))
    dense = measure_scene(engine, scene, push, a, orders)
    y = yardstick(engine, scene, push, a)
    dense["yardstick_primary_ms"] = y
    for k, v in dense.items():
        if isinstance(v, dict) and "rays_per_s" in v:
            v["ratio_to_yardstick_on"] = v["median_ms"] / y["tags_and_sky_fast_on"]["median_ms"]
            v["ratio_to_yardstick_off"] = v["median_ms"] / y["tags_and_sky_fast_off"]["median_ms"]
    extra = W * H * (8 + 6)
    allowance = y["tags_and_sky_fast_off"]["median_ms"] + extra / HBM_BYTES_PER_S * 1e3
    dense["pick_block_vs_yardstick"] = {"extra_bytes": extra, "hbm_bytes_per_s": HBM_BYTES_PER_S, "allowance_ms": allowance,
                                        "pick_block8x8_ms": dense["pick_block8x8"]["median_ms"],
                                        "needs_explanation": dense["pick_block8x8"]["median_ms"] > allowance}
    result["scenes"]["treehouse_256"] = dense
    scene.destroy()

    if not a.no_bricks:
        N = 2048
        grid, pool = vrt.synthetic.sparse_brick_scene(N, 0.015, seed=5)
        scene = vrt.VoxelScene.from_bricks(engine, grid, pool, pal)
        pos, yaw, pitch = vrt.synthetic.default_camera_for(N, N, N)
        push = vrt.make_push(vrt.CameraController(position=pos, yaw=yaw, pitch=pitch), (N, N, N), (W, H))
        result["scenes"]["sparse_bricks_2048"] = measure_scene(engine, scene, push, a, orders)
        scene.destroy()

    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
