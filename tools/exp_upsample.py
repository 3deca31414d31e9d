"""Temporal upsampling (vrt_upsample, k_upsample) timed at 1129x635 -> 1920x1080 and 1920x1080 -> 3840x2160 on moving poses of the
fly-through (tools/flythrough.py: the treehouse scene, reference defaults), beside the path it replaces: vrt_reproject at render
size plus the vrt_blit to the display -- in the same process, alternating.
   python tools/exp_upsample.py [--frames N] [--reps R] [--out profiles/upsample_times.json]
   python tools/exp_upsample.py --camera perspective:FOV|ortho:HW|panorama [--out profiles/upsample_cam_times.json]
--camera: vrt_upsample_camera (k_upsample_cam<MODEL>) at 960x540 -> 1920x1080 on frames drawn through that ray camera -- the jitter
sequence as camera_jitter (perspective) or as sample offsets (vrt_camera_rays_offset) --, beside vrt_upsample (k_upsample) on the
same planes and the same history in the same process, alternating, with the spread of each kernel's per-frame medians; several
--camera runs add their entries to one file.
HIP events, warm-up, median of R (default 20) per pose, median over the poses.  Every timed call works on the history of the
frame before, of a camera that moved, so the gather is the moving case's.  The byte accounting is the kernel's own
(csrc/vrt_upsample.hip), per DISPLAY pixel at scale s: 24 / s^2 B of current planes, at most 96 B of history in (24 B of it from
HBM where neighbouring lanes' taps are neighbouring texels -- both are reported), 36 B out; the implied TB/s is that over the
median time.  No speed bar: the kernel keeps a history at display size, which the pair it replaces does not.  Reported numbers,
not gates."""
import argparse, ctypes as C, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import voxel_raytracing_amd as vrt

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=8)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "upsample_times.json"))
ap.add_argument("--camera", default=None, help="perspective:FOV | ortho:HALFWIDTH | panorama")
args = ap.parse_args()
if args.camera and args.out.endswith("upsample_times.json"):
    args.out = os.path.join(os.path.dirname(args.out), "upsample_cam_times.json")
if args.camera and args.camera.partition(":")[0] not in ("perspective", "ortho", "panorama"):
    sys.exit("--camera perspective:FOV | ortho:HALFWIDTH | panorama")
ACHIEVABLE_TBS = 6.3
eng = vrt.Engine(0)
lib = vrt.lib()
sc = vrt.VoxelScene.from_dense(eng, vrt.synthetic.treehouse(256, seed=2), vrt.synthetic.default_palette(metallic_ids=range(200, 256)),
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
    """vrt_upsample_camera against vrt_upsample on the same frames: per frame the median of 2 x `reps` calls of each, alternating."""
    TW, TH = 1920, 1080
    kind, _, value = args.camera.partition(":")
    st = vrt.VoxelRenderSettings(targetResolution=(TW, TH)); st.fsrSetttings.scaling = vrt.FsrScaling.PERFORMANCE
    W, H = st.renderResolution()
    assert (W, H) == (960, 540), (W, H)
    r = vrt.VoxelRenderer(eng, st, sc)
    pos, yaw, pitch = vrt.synthetic.default_camera_for(sc.width, sc.height, sc.depth)
    ctrl = vrt.CameraController(position=pos, yaw=yaw, pitch=pitch)
    if kind == "perspective": cam = vrt.RayCamera.perspective(ctrl, float(value))
    elif kind == "ortho": cam = vrt.RayCamera.orthographic(ctrl, float(value))
    else: cam = vrt.RayCamera.panorama(tuple(ctrl.position))
    dev = eng.torch_device
    hist = [(torch.zeros((TH, TW, 4), dtype=torch.int16, device=dev), torch.zeros((TH, TW, 4), dtype=torch.int32, device=dev)) for _ in range(3)]
    resolved = torch.zeros((TH, TW, 4), dtype=torch.uint8, device=dev); motion = torch.zeros((TH, TW, 2), dtype=torch.float32, device=dev)
    phases = int(lib.vrt_jitter_phase_count(W, TW))
    t_cam, t_pin, valid, prev_c, prev_p, cur_h = [], [], [], None, None, -1
    for f in range(args.frames):
        ctrl.mouse(0.25, 0.0); ctrl.update(1.0 / 60.0, 0.1, 0.2)
        if kind == "panorama": cam.camera = vrt.CameraController(position=tuple(ctrl.position))
        jx, jy = C.c_float(), C.c_float()
        vrt._capi.check(lib.vrt_jitter_offset(f % phases, phases, C.byref(jx), C.byref(jy)))
        j = (jx.value, jy.value)
        cc = cam.to_c((W, H)); push = vrt.make_push(ctrl, (sc.width, sc.height, sc.depth), (W, H), f + 1)     # the pass's cameras: no jitter, no offset
        o, d = cam.rays(eng, (W, H), j) if kind == "perspective" else cam.rays(eng, (W, H), offset=j)
        gb = r._geometryStage.record_rays(o, d, (W, H), f + 1)
        color = r._denoiserStage.record(gb.color, gb.normal, gb.position)
        rs = vrt._capi.ReprojectSettings(); lib.vrt_upsample_camera_settings_default(C.byref(cc), W, C.byref(rs))
        nxt = (cur_h + 1) % 2 if cur_h >= 0 else 0
        hout = vrt._capi.History(hist[nxt][0].data_ptr(), hist[nxt][1].data_ptr())
        hin = vrt._capi.History(hist[cur_h][0].data_ptr(), hist[cur_h][1].data_ptr()) if cur_h >= 0 else None
        tmp = vrt._capi.History(hist[2][0].data_ptr(), hist[2][1].data_ptr())       # the timed calls write a third pair
        args_ = (color.data_ptr(), gb.position.data_ptr(), gb.normal.data_ptr())
        if hin is not None:
            f_cam = lambda: lib.vrt_upsample_camera(eng.ctx, W, H, TW, TH, C.byref(cc), C.byref(prev_c), C.byref(rs), *args_, C.byref(hin), C.byref(tmp), resolved.data_ptr(), motion.data_ptr())
            f_pin = lambda: lib.vrt_upsample(eng.ctx, W, H, TW, TH, C.byref(push), C.byref(prev_p), C.byref(rs), *args_, C.byref(hin), C.byref(tmp), resolved.data_ptr(), motion.data_ptr())
            vrt._capi.check(f_cam()); vrt._capi.check(f_pin())
            a, b = timed(f_pin, args.reps), timed(f_cam, args.reps)
            t_pin.append(statistics.median([a, timed(f_pin, args.reps)])); t_cam.append(statistics.median([b, timed(f_cam, args.reps)]))
        vrt._capi.check(lib.vrt_upsample_camera(eng.ctx, W, H, TW, TH, C.byref(cc), C.byref(prev_c if prev_c is not None else cc), C.byref(rs), *args_,
                                                C.byref(hin) if hin is not None else None, C.byref(hout), resolved.data_ptr(), motion.data_ptr()))
        torch.cuda.synchronize()
        valid.append(float(((hist[nxt][1][..., 3].cpu().numpy().view(np.uint32) >> 24) > 1).mean()))
        cur_h, prev_c, prev_p = nxt, cc, push
    entry = {"k_upsample_cam_us": statistics.median(t_cam), "k_upsample_same_planes_us": statistics.median(t_pin),
             "k_upsample_frame_medians_min_max_us": [min(t_pin), max(t_pin)], "k_upsample_cam_frame_medians_min_max_us": [min(t_cam), max(t_cam)],
             "pixels_with_history": statistics.median(valid[1:]), "frames": args.frames, "reps": args.reps, "size": f"{W}x{H}->{TW}x{TH}"}
    out = {}
    if os.path.exists(args.out):
        with open(args.out) as fh:
            out = json.load(fh)
    out["device"] = eng.device_info()[0]; out.setdefault("cameras", {})[args.camera] = entry
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(args.camera, json.dumps(entry)); print("wrote", args.out)


eng.set_timing(False)
if args.camera:
    camera_run()
    sys.exit(0)
result = {"device": eng.device_info()[0], "achievable_tbs": ACHIEVABLE_TBS, "sizes": {}}
for (TW, TH), scaling in (((1920, 1080), vrt.FsrScaling.BALANCED), ((3840, 2160), vrt.FsrScaling.PERFORMANCE)):
    st = vrt.VoxelRenderSettings(targetResolution=(TW, TH)); st.fsrSetttings.scaling = scaling
    W, H = st.renderResolution()
    r = vrt.VoxelRenderer(eng, st, sc, temporal=True, reproject=True, upsample=True)
    pos, yaw, pitch = vrt.synthetic.default_camera_for(sc.width, sc.height, sc.depth)
    r.camera.position = np.array(pos, np.float32); r.camera.yaw, r.camera.pitch = yaw, pitch; r.camera.updateDirectionVectors()
    up, dev = r.upscaler, eng.torch_device
    lo = vrt.UpscalerStage(eng, st)                                               # the replaced path, fed the same frames
    spare = [(torch.zeros((H, W, 4), dtype=torch.int16, device=dev), torch.zeros((H, W, 4), dtype=torch.int32, device=dev)),
             (torch.zeros((TH, TW, 4), dtype=torch.int16, device=dev), torch.zeros((TH, TW, 4), dtype=torch.int32, device=dev))]
    res_lo = torch.zeros((H, W, 4), dtype=torch.uint8, device=dev); res_hi = torch.zeros((TH, TW, 4), dtype=torch.uint8, device=dev)
    mot_hi = torch.zeros((TH, TW, 2), dtype=torch.float32, device=dev)
    t_up, t_pair, valid = [], [], []
    prev = None
    for f in range(args.frames):                                                  # W + D while turning, as the fly-through's middle third
        r.camera.mouse(0.25, 0.0); r.update(1.0 / 60.0, 0.1, 0.2)
        push = r.push_constants()
        gb = r._geometryStage.record(push)
        color = r._denoiserStage.record(gb.color, gb.normal, gb.position)
        if prev is not None:
            rs = up.reprojectSettings.to_c(push)
            hin_hi, hin_lo = up.next_histories()[0], lo.next_histories()[0]
            hout_lo = vrt._capi.History(spare[0][0].data_ptr(), spare[0][1].data_ptr())
            hout_hi = vrt._capi.History(spare[1][0].data_ptr(), spare[1][1].data_ptr())
            f_up = lambda: lib.vrt_upsample(eng.ctx, W, H, TW, TH, C.byref(push), C.byref(prev), C.byref(rs), color.data_ptr(), gb.position.data_ptr(),
                                            gb.normal.data_ptr(), C.byref(hin_hi), C.byref(hout_hi), res_hi.data_ptr(), mot_hi.data_ptr())
            f_pair = lambda: (lib.vrt_reproject(eng.ctx, W, H, C.byref(push), C.byref(prev), C.byref(rs), color.data_ptr(), gb.position.data_ptr(),
                                                gb.normal.data_ptr(), C.byref(hin_lo), C.byref(hout_lo), res_lo.data_ptr(), gb.motion.data_ptr()),
                              lib.vrt_blit(eng.ctx, res_lo.data_ptr(), W, H, res_hi.data_ptr(), TW, TH))
            a, b = [], []
            for _ in range(2):                                                    # alternating
                a.append(timed(f_up, args.reps // 2)); b.append(timed(f_pair, args.reps // 2))
            t_up.append(statistics.median(a)); t_pair.append(statistics.median(b))
        up.record_upsampled(color, gb, push)
        lo.record_reprojected(color, gb, push)
        torch.cuda.synchronize()
        valid.append(float(((up.history()[1][..., 3] >> 24) > 1).mean()))
        prev = vrt._capi.Push.from_buffer_copy(push)
    s2 = (TW * TH) / (W * H)
    bytes_px = {"current_planes": 24 / s2, "history_in_max": 96, "history_in_hbm": 24, "out": 36}
    us = statistics.median(t_up)
    tbs_max = TW * TH * (bytes_px["current_planes"] + 96 + 36) / (us * 1e-6) / 1e12
    tbs_hbm = TW * TH * (bytes_px["current_planes"] + 24 + 36) / (us * 1e-6) / 1e12
    result["sizes"][f"{W}x{H}->{TW}x{TH}"] = {"k_upsample_us": us, "reproject_plus_blit_us": statistics.median(t_pair), "bytes_per_display_pixel": bytes_px,
                                            "implied_tbs_all_taps": tbs_max, "implied_tbs_hbm": tbs_hbm, "fraction_of_achievable_hbm": tbs_hbm / ACHIEVABLE_TBS,
                                            "pixels_with_history": statistics.median(valid[1:]), "frames": args.frames, "reps": args.reps}
    print(f"{W}x{H} -> {TW}x{TH}: k_upsample {us:.1f} us ({tbs_hbm:.2f} TB/s from HBM by its own accounting, {tbs_max:.2f} with every tap); "
          f"vrt_reproject + vrt_blit {statistics.median(t_pair):.1f} us; {statistics.median(valid[1:]):.2f} of the pixels kept history", flush=True)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(result, fh, indent=1)
print("wrote", args.out)
