"""Scripted fly-through: replays keyboard / mouse input through CameraController (camera_controller.cpp:30-68)
and renders every frame through the whole frame graph of voxel_renderer.cpp:55-94 -- geometry (reference defaults: AO 4,
shadow, <= 5 bounces), 2 denoiser passes, jittered accumulation stand-in for FSR2 at the BALANCED render scale, window blit.
   python tools/flythrough.py [--frames N] [--png-dir DIR] [--vox FILE] [--reproject [--upsample] [--projection perspective:FOV|ortho:HW|panorama]]
--reproject keeps the history across the moving frames by temporal reprojection (vrt_reproject) instead of dropping it every frame;
--upsample (with --reproject) keeps that history at the target resolution (vrt_upsample) instead of blitting a render-resolution one.
--projection (with --reproject) draws the frames through that ray camera, which follows the scripted controller, and keeps the history by
vrt_reproject_camera -- with --upsample too, at the target resolution by vrt_upsample_camera (the jitter sequence as sample offsets).
Prints frame-time statistics measured with HIP events over the whole run (no per-frame synchronisation)."""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import voxel_raytracing_amd as vrt

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=240)
ap.add_argument("--png-dir", default=None)
ap.add_argument("--vox", default=None)
ap.add_argument("--target", default="1920x1080")
ap.add_argument("--reproject", action="store_true")
ap.add_argument("--upsample", action="store_true")
ap.add_argument("--projection", default=None, help="perspective:FOV | ortho:HALFWIDTH | panorama (needs --reproject)")
args = ap.parse_args()
TW, TH = (int(v) for v in args.target.split("x"))
eng = vrt.Engine(0)
if args.vox:
    sc = vrt.VoxelScene(eng, args.vox); N = max(sc.width, sc.height, sc.depth)
else:
    N = 256
    sc = vrt.VoxelScene.from_dense(eng, vrt.synthetic.treehouse(N, seed=2), vrt.synthetic.default_palette(metallic_ids=range(200, 256)),
                                   sky=vrt.synthetic.sky_gradient(512, 256), noise=vrt.synthetic.blue_noise_standin(512))
st = vrt.VoxelRenderSettings(targetResolution=(TW, TH))                      # reference defaults incl. FSR BALANCED render scale
pos, yaw, pitch = vrt.synthetic.default_camera_for(sc.width, sc.height, sc.depth)
cam = None
if args.projection:
    kind, _, value = args.projection.partition(":")
    ctrl = vrt.CameraController(position=pos, yaw=yaw, pitch=pitch)
    if kind == "perspective" and value: cam = vrt.RayCamera.perspective(ctrl, float(value))
    elif kind == "ortho" and value: cam = vrt.RayCamera.orthographic(ctrl, float(value))
    elif kind == "panorama" and not value: cam = vrt.RayCamera.panorama(pos)
    else: sys.exit("--projection perspective:FOV | ortho:HALFWIDTH | panorama")
r = vrt.VoxelRenderer(eng, st, sc, temporal=True, windowSize=(TW, TH), reproject=args.reproject, upsample=args.upsample, camera=cam)
if cam is not None:
    r._camera = cam.camera                                                   # the scripted input drives the ray camera's controller
r.camera.position = np.array(pos, np.float32); r.camera.yaw, r.camera.pitch = yaw, pitch; r.camera.updateDirectionVectors()
third = max(1, args.frames // 3)
keys = [vrt.CameraKey(frames=third, forward=1.0),                            # W
        vrt.CameraKey(frames=third, forward=0.5, strafe=1.0, mouseX=0.25),   # W + D while turning
        vrt.CameraKey(frames=args.frames - 2 * third, forward=-0.5, mouseX=-0.4, mouseY=0.1)]
RW, RH = st.renderResolution()
print(f"scene {sc.width}x{sc.height}x{sc.depth}, render {RW}x{RH} -> target {TW}x{TH}, {args.frames} frames", flush=True)
eng.set_timing(False)
for _ in range(3):
    r.update(0.0); r.render()
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
t0 = time.perf_counter(); e0.record()
f = 0
for k in keys:
    for _ in range(k.frames):
        if k.mouseX or k.mouseY: r.camera.mouse(k.mouseX, k.mouseY)
        r.update(1.0 / 60.0, k.forward * 0.2, k.strafe * 0.2)               # VoxelRenderer::update: camera + jitter sequence
        if not args.reproject:
            r.upscaler.reset()                                               # moving camera, no reprojection: one frame of history
        img = r.render()
        if args.png_dir and f % 20 == 0:
            os.makedirs(args.png_dir, exist_ok=True)
            vrt.write_image(os.path.join(args.png_dir, f"frame_{f:04d}.png"), img.cpu().numpy())
        f += 1
e1.record(); torch.cuda.synchronize()
wall = time.perf_counter() - t0
gpu_ms = e0.elapsed_time(e1)
rays = RW * RH * args.frames
print(f"GPU {gpu_ms / args.frames * 1e3:.1f} us/frame ({args.frames / gpu_ms * 1e3:.0f} frames/s, {rays / gpu_ms / 1e3:.0f} primary Mrays/s); host wall {wall / args.frames * 1e3:.3f} ms/frame")
print("final camera", r.camera.position.tolist(), r.camera.yaw, r.camera.pitch)
