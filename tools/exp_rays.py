"""vrt_render_rays timed at 1920x1080 on the treehouse stand-in with the pinhole's rays and the reference defaults, beside the two
paths that draw the same frame with the built-in camera -- in one process, alternating:
   (a) vrt_render_geometry, the default path (the megakernel);
   (b) vrt_render_geometry with VRT_FLAG_SPLIT_KERNELS (K1 MODE 0 -> records -> K2);
   (c) vrt_camera_rays + vrt_render_rays (both calls timed together), and vrt_render_rays alone on rays made beforehand.
   python tools/exp_rays.py [--reps R] [--out profiles/render_rays_times.json]
HIP events around the calls, 3 warm-up launches, R (default 20) repetitions in 3 rounds that alternate the paths; per path the median,
the minimum and the maximum over all repetitions.  (a) and (b) are the yardsticks, measured by this same run; the new path is
never its own.  The frames are checked to be the same picture (color8 of (c) == (a)) before anything is timed.  Reported numbers,
not gates: this path writes and re-reads 16 B per hit, reads 24 B per ray and shades from the hit stack, not the packed chain."""
import argparse, ctypes as C, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import voxel_raytracing_amd as vrt

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "render_rays_times.json"))
args = ap.parse_args()
W, H = 1920, 1080
eng = vrt.Engine(0)
lib = vrt.lib()
sc = vrt.VoxelScene.from_dense(eng, vrt.synthetic.treehouse(256, seed=2), vrt.synthetic.default_palette(metallic_ids=range(200, 256)),
                               sky=vrt.synthetic.sky_gradient(512, 256), noise=vrt.synthetic.blue_noise_standin(512))
st = vrt.VoxelRenderSettings(targetResolution=(W, H)); st.fsrSetttings.enable = False
pos, yaw, pitch = vrt.synthetic.default_camera_for(sc.width, sc.height, sc.depth)
ctl = vrt.CameraController(position=pos, yaw=yaw, pitch=pitch)
push = vrt.make_push(ctl, (sc.width, sc.height, sc.depth), (W, H), 3)
cam = vrt.RayCamera.perspective(ctl, 90.0)
stage = vrt.GeometryStage(eng, st, sc)
st_split = vrt.VoxelRenderSettings(targetResolution=(W, H)); st_split.fsrSetttings.enable = False; st_split.traceSettings.splitKernels = True
stage_split = vrt.GeometryStage(eng, st_split, sc)
stage_rays = vrt.GeometryStage(eng, st, sc)
o, d = cam.rays(eng, (W, H))

# the same picture three ways
a = stage.record(push).color.clone(); b = stage_split.record(push).color.clone(); c = stage_rays.record_rays(o, d, (W, H), frame=3).color.clone()
eng.synchronize()
same = bool((a == b).all().item() and (a == c).all().item())

paths = {
    "a_render_geometry": lambda: stage.record(push),
    "b_render_geometry_split": lambda: stage_split.record(push),
    "c_camera_rays_plus_render_rays": lambda: stage_rays.record_rays(*cam.rays(eng, (W, H)), (W, H), frame=3),
    "c_render_rays_alone": lambda: stage_rays.record_rays(o, d, (W, H), frame=3),
}
eng.set_timing(False)
ms = {k: [] for k in paths}
for fn in paths.values():
    for _ in range(3):
        fn()
torch.cuda.synchronize()
rounds = 3
for r in range(rounds):
    for k, fn in paths.items():
        for _ in range(-(-args.reps // rounds)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1))
result = {"device": eng.device_info()[0], "scene": "treehouse(256, seed=2)", "resolution": [W, H], "settings": "reference defaults, frame 3",
          "same_picture": same, "reps": len(next(iter(ms.values()))),
          "us": {k: {"median": statistics.median(v) * 1e3, "min": min(v) * 1e3, "max": max(v) * 1e3} for k, v in ms.items()}}
print(json.dumps(result, indent=1))
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(result, f, indent=1); f.write("\n")
