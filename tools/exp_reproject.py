"""Temporal reprojection (vrt_reproject, k_reproject) timed at 1080p and 4K on poses of the fly-through (tools/flythrough.py: the
treehouse scene, reference defaults), beside what it is compared with: the accumulation pair it replaces (vrt_accumulate +
vrt_resolve) and the two denoiser passes that run before it.
   python tools/exp_reproject.py [--frames N] [--reps R] [--out profiles/reproject_times.json]
   python tools/exp_reproject.py --camera perspective:FOV|ortho:HW|panorama [--out profiles/reproject_cam_times.json]
--camera: vrt_reproject_camera (k_reproject_cam) at 1080p on frames drawn through that ray camera, beside vrt_reproject
(k_reproject) on the same planes in the same process, with the spread of k_reproject's own per-frame medians; several --camera
runs add their entries to one file.
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
ap.add_argument("--camera", default=None, help="perspective:FOV | ortho:HALFWIDTH | panorama")
args = ap.parse_args()
if args.camera and args.out.endswith("reproject_times.json"):
    args.out = os.path.join(os.path.dirname(args.out), "reproject_cam_times.json")
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




def camera_run():
    """vrt_reproject_camera against vrt_reproject on the same frames: per frame the median of `reps` calls of each, alternating."""
    W, H = 1920, 1080
    kind, _, value = args.camera.partition(":")
    st = vrt.VoxelRenderSettings(targetResolution=(W, H)); st.fsrSetttings.enable = False
    r = vrt.VoxelRenderer(eng, st, sc)
    pos, yaw, pitch = vrt.synthetic.default_camera_for(sc.width, sc.height, sc.depth)
    ctrl = vrt.CameraController(position=pos, yaw=yaw, pitch=pitch)
    if kind == "perspective": cam = vrt.RayCamera.perspective(ctrl, float(value))
    elif kind == "ortho": cam = vrt.RayCamera.orthographic(ctrl, float(value))
    elif kind == "panorama": cam = vrt.RayCamera.panorama(tuple(ctrl.position))
    else: sys.exit("--camera perspective:FOV | ortho:HALFWIDTH | panorama")
    dev = eng.torch_device
    hist = [(torch.zeros((H, W, 4), dtype=torch.int16, device=dev), torch.zeros((H, W, 4), dtype=torch.int32, device=dev)) for _ in range(3)]
    resolved = torch.zeros((H, W, 4), dtype=torch.uint8, device=dev); motion = torch.zeros((H, W, 2), dtype=torch.float32, device=dev)
    t_cam, t_pin, valid, prev_c, prev_p, cur_h = [], [], [], None, None, -1
    for f in range(args.frames):
        ctrl.mouse(0.25, 0.0); ctrl.update(1.0 / 60.0, 0.1, 0.2)
        if kind == "panorama": cam.camera = vrt.CameraController(position=tuple(ctrl.position))
        cc = cam.to_c((W, H)); push = vrt.make_push(ctrl, (sc.width, sc.height, sc.depth), (W, H), f + 1)
        o, d = cam.rays(eng, (W, H))
        gb = r._geometryStage.record_rays(o, d, (W, H), f + 1)
        color = r._denoiserStage.record(gb.color, gb.normal, gb.position)
        rs = vrt._capi.ReprojectSettings(); lib.vrt_reproject_camera_settings_default(C.byref(cc), W, C.byref(rs))
        nxt = (cur_h + 1) % 2 if cur_h >= 0 else 0
        hout = vrt._capi.History(hist[nxt][0].data_ptr(), hist[nxt][1].data_ptr())
        hin = vrt._capi.History(hist[cur_h][0].data_ptr(), hist[cur_h][1].data_ptr()) if cur_h >= 0 else None
        tmp = vrt._capi.History(hist[2][0].data_ptr(), hist[2][1].data_ptr())       # the timed calls write a third pair
        args_ = (color.data_ptr(), gb.position.data_ptr(), gb.normal.data_ptr())
        if hin is not None:
            f_cam = lambda: lib.vrt_reproject_camera(eng.ctx, W, H, C.byref(cc), C.byref(prev_c), C.byref(rs), *args_, C.byref(hin), C.byref(tmp), resolved.data_ptr(), motion.data_ptr())
            f_pin = lambda: lib.vrt_reproject(eng.ctx, W, H, C.byref(push), C.byref(prev_p), C.byref(rs), *args_, C.byref(hin), C.byref(tmp), resolved.data_ptr(), motion.data_ptr())
            a, b = timed(f_pin, args.reps), timed(f_cam, args.reps)
            t_pin.append(statistics.median([a, timed(f_pin, args.reps)])); t_cam.append(statistics.median([b, timed(f_cam, args.reps)]))
        vrt._capi.check(lib.vrt_reproject_camera(eng.ctx, W, H, C.byref(cc), C.byref(prev_c if prev_c is not None else cc), C.byref(rs), *args_,
                                                 C.byref(hin) if hin is not None else None, C.byref(hout), resolved.data_ptr(), motion.data_ptr()))
        torch.cuda.synchronize()
        valid.append(float(((hist[nxt][1][..., 3].cpu().numpy().view(np.uint32) >> 24) > 1).mean()))
        cur_h, prev_c, prev_p = nxt, cc, push
    entry = {"k_reproject_cam_us": statistics.median(t_cam), "k_reproject_same_planes_us": statistics.median(t_pin),
             "k_reproject_frame_medians_min_max_us": [min(t_pin), max(t_pin)], "k_reproject_cam_frame_medians_min_max_us": [min(t_cam), max(t_cam)],
             "pixels_with_history": statistics.median(valid[1:]), "frames": args.frames, "reps": args.reps, "size": f"{W}x{H}"}
    out = {}
    if os.path.exists(args.out):
        with open(args.out) as fh:
            out = json.load(fh)
    out["device"] = eng.device_info()[0]; out.setdefault("cameras", {})[args.camera] = entry
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(args.camera, json.dumps(entry)); print("wrote", args.out)


if args.camera:
    eng.set_timing(False)
    camera_run()
    sys.exit(0)
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
            hin, hout = up.next_histories()
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
