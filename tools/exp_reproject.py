"""Temporal reprojection (vrt_reproject, k_reproject) timed at 1080p and 4K on poses of the fly-through (tools/flythrough.py: the
treehouse scene, reference defaults), beside what it is compared with: the accumulation pair it replaces (vrt_accumulate +
vrt_resolve) and the two denoiser passes that run before it.
   python tools/exp_reproject.py [--frames N] [--reps R] [--out profiles/reproject_times.json]
HIP events, warm-up, medians.  Every timed call reprojects frame k onto the history of frame k - 1 of a camera that moved
between them, so the gather is the moving case's.  The byte accounting is the kernel's own (csrc/vrt_reproject.hip): 24 B/px of
current planes, 24 B/px of history in, 36 B/px out = 84 B/px; the implied TB/s is that over the median time.  Reported numbers,
not gates."""
import argparse, ctypes as C, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import voxel_raytracing_amd as vrt

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=12)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "reproject_times.json"))
args = ap.parse_args()
BYTES = {"current_planes": 24, "history_in": 24, "out": 36}
ACHIEVABLE_TBS = 6.3
eng = vrt.Engine(0)
lib = vrt.lib()
N = 256
sc = vrt.VoxelScene.from_dense(eng, vrt.synthetic.treehouse(N, seed=2), vrt.synthetic.default_palette(metallic_ids=range(200, 256)),
                               sky=vrt.synthetic.sky_gradient(512, 256), noise=vrt.synthetic.blue_noise_standin(512))


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms) * 1e3          # us


result = {"device": eng.device_info()[0], "bytes_per_pixel": dict(BYTES, total=sum(BYTES.values())), "achievable_tbs": ACHIEVABLE_TBS, "sizes": {}}
eng.set_timing(False)
for W, H in ((1920, 1080), (3840, 2160)):
    st = vrt.VoxelRenderSettings(targetResolution=(W, H)); st.fsrSetttings.enable = False
    r = vrt.VoxelRenderer(eng, st, sc, temporal=True, reproject=True)
    pos, yaw, pitch = vrt.synthetic.default_camera_for(sc.width, sc.height, sc.depth)
    r.camera.position = np.array(pos, np.float32); r.camera.yaw, r.camera.pitch = yaw, pitch; r.camera.updateDirectionVectors()
    up, dev = r.upscaler, eng.torch_device
    t_rep, t_acc, t_den, valid = [], [], [], []
    accum = torch.zeros((H, W, 4), dtype=torch.int32, device=dev); res = torch.zeros((H, W, 4), dtype=torch.uint8, device=dev)
    prev = None
    for f in range(args.frames):                                                  # W + D while turning, as the fly-through's middle third
        r.camera.mouse(0.25, 0.0); r.update(1.0 / 60.0, 0.1, 0.2)
        push = r.push_constants()
        gb = r._geometryStage.record(push)
        color = r._denoiserStage.record(gb.color, gb.normal, gb.position)
        if prev is not None:
            hin = vrt._capi.History(up._hist[up._hist_cur][0].data_ptr(), up._hist[up._hist_cur][1].data_ptr())
            o = 1 - up._hist_cur
            hout = vrt._capi.History(up._hist[o][0].data_ptr(), up._hist[o][1].data_ptr())
            rs = up.reprojectSettings.to_c(push)
            t_rep.append(timed(lambda: lib.vrt_reproject(eng.ctx, W, H, C.byref(push), C.byref(prev), C.byref(rs), color.data_ptr(), gb.position.data_ptr(),
                                                         gb.normal.data_ptr(), C.byref(hin), C.byref(hout), up._resolved.data_ptr(), gb.motion.data_ptr()), args.reps))
            t_acc.append(timed(lambda: (lib.vrt_accumulate(eng.ctx, color.data_ptr(), accum.data_ptr(), W, H, 1),
                                        lib.vrt_resolve(eng.ctx, accum.data_ptr(), res.data_ptr(), W, H, 1)), args.reps))
            t_den.append(timed(lambda: r._denoiserStage.record(gb.color, gb.normal, gb.position), args.reps))
        up.record_reprojected(color, gb, push)
        torch.cuda.synchronize()
        valid.append(float(((up.history()[1][..., 3] >> 24) > 1).mean()))
        prev = vrt._capi.Push.from_buffer_copy(push)
    us = statistics.median(t_rep)
    tbs = W * H * sum(BYTES.values()) / (us * 1e-6) / 1e12
    result["sizes"][f"{W}x{H}"] = {"k_reproject_us": us, "accumulate_resolve_us": statistics.median(t_acc), "denoise_2_passes_us": statistics.median(t_den),
                                   "implied_tbs": tbs, "fraction_of_achievable": tbs / ACHIEVABLE_TBS, "pixels_with_history": statistics.median(valid[1:]),
                                   "frames": args.frames, "reps": args.reps}
    print(f"{W}x{H}: k_reproject {us:.1f} us ({tbs:.2f} TB/s by its own accounting, {tbs / ACHIEVABLE_TBS:.2f} of {ACHIEVABLE_TBS}); "
          f"accumulate + resolve {statistics.median(t_acc):.1f} us; denoiser {statistics.median(t_den):.1f} us; "
          f"{statistics.median(valid[1:]):.2f} of the pixels kept history", flush=True)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(result, fh, indent=1)
print("wrote", args.out)
