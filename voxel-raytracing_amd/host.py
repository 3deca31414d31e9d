"""Host-side mirror of the reference's call surface for the hot path (Python over the C-ABI).

Same names, argument meaning and error behaviour as the reference objects (paths relative to the
reference root):

  VoxelRenderSettings   source/voxels/voxel_render_settings.hpp:6-59, .cpp:3-13
  CameraController      source/voxels/resource/camera_controller.cpp:15-28
  VoxelScene            source/voxels/resource/voxel_scene.hpp:18-34, .cpp:33-133
  GeometryStage         source/voxels/stages/geometry_stage.hpp:19-53, .cpp:106-153
  DenoiserStage         source/voxels/stages/denoiser_stage.hpp:22-47, .cpp:143-258
  VoxelRenderer         source/voxels/voxel_renderer.hpp:17-38, .cpp:16-94
  Engine                source/engine/engine.hpp:71-76 (reduced to: device + stream)

torch is used only for device buffers and the stream; every computation goes through libvrt_hip.so.
"""
import ctypes as C
import enum
import math
import os
from dataclasses import dataclass, field
from typing import Optional, Tuple

import numpy as np

from . import _capi
from ._capi import check, lib


# --------------------------------------------------------------------------------------------------
# settings (voxel_render_settings.hpp)
# --------------------------------------------------------------------------------------------------

class FsrScaling(enum.IntEnum):          # :6-13
    NONE = 10
    QUALITY = 15
    BALANCED = 17
    PERFORMANCE = 20
    ULTRA_PERFORMANCE = 30


@dataclass
class FsrSettings:                       # :15-19  (FSR2 itself is out of scope; only the render scale applies)
    enable: bool = True
    scaling: FsrScaling = FsrScaling.BALANCED


@dataclass
class DenoiserSettings:                  # :21-29
    enable: bool = True
    iterations: int = 2
    phiColor0: float = 20.4
    phiNormal0: float = 1e-2
    phiPos0: float = 1e-1
    stepWidth: float = 2.0
    mode: int = _capi.DENOISE_CANONICAL  # build extension: as-shipped std140 aliasing mode


@dataclass
class AmbientOcclusionSettings:          # :31-35
    numSamples: int = 4
    intensity: float = 1.0


def _norm111():
    v = np.float32(1.0) / np.sqrt(np.float32(3.0))
    return (float(v), float(v), float(v))


@dataclass
class LightSettings:                     # :37-42
    direction: Tuple[float, float, float] = field(default_factory=_norm111)
    color: Tuple[float, float, float, float] = (1.0, 1.0, 1.0, 1.0)
    intensity: float = 1.0


@dataclass
class TraceSettings:
    """The shader's compile-time constants (voxel_volume.frag:68-69,219) as runtime knobs."""
    maxRaySteps: int = 512
    aoSteps: int = 64
    maxReflections: int = 5
    shadows: bool = True
    traversal: int = _capi.TRAVERSAL_AUTO
    splitKernels: bool = False         # K1 + K2 over the compacted hit list instead of the megakernel


@dataclass
class ReprojectSettings:
    """vrt_reproject_settings: how temporal reprojection accepts and weighs history (include/vrt.h)."""
    maxHistory: int = 32               # 1..255 frames
    tolAbs: float = 0.5                # voxels
    tolRel: Optional[float] = None     # voxels per unit of depth; None: two pixel footprints of the push it is used with

    def over(self, s: _capi.ReprojectSettings) -> _capi.ReprojectSettings:
        """`s`, the defaults of some camera, overridden by what is set here."""
        s.max_history, s.tol_abs = int(self.maxHistory), float(self.tolAbs)
        if self.tolRel is not None:
            s.tol_rel = float(self.tolRel)
        return s

    def to_c(self, push: _capi.Push) -> _capi.ReprojectSettings:
        s = _capi.ReprojectSettings()
        lib().vrt_reproject_settings_default(C.byref(push), C.byref(s))
        return self.over(s)


def _scale(scaling: FsrScaling, dim: int) -> int:      # voxel_render_settings.cpp:3-6
    return int(np.float32(np.float32(10.0) / np.float32(int(scaling))) * np.float32(dim))


@dataclass
class VoxelRenderSettings:               # :44-59
    targetResolution: Tuple[int, int] = (1920, 1080)
    fsrSetttings: FsrSettings = field(default_factory=FsrSettings)       # (sic) reference spelling
    denoiserSettings: DenoiserSettings = field(default_factory=DenoiserSettings)
    occlusionSettings: AmbientOcclusionSettings = field(default_factory=AmbientOcclusionSettings)
    lightSettings: LightSettings = field(default_factory=LightSettings)
    traceSettings: TraceSettings = field(default_factory=TraceSettings)
    voxPath: str = "../resource/treehouse.vox"
    skyboxPath: str = "../resource/rustig_koppie.hdr"

    def renderResolution(self) -> Tuple[int, int]:     # voxel_render_settings.cpp:8-13
        if self.fsrSetttings.enable:
            return (_scale(self.fsrSetttings.scaling, self.targetResolution[0]),
                    _scale(self.fsrSetttings.scaling, self.targetResolution[1]))
        return tuple(self.targetResolution)

    def to_c(self) -> _capi.Settings:
        s = _capi.Settings()
        s.ao_samples = int(self.occlusionSettings.numSamples)          # geometry_stage.cpp:135
        s.ambient_intensity = float(self.occlusionSettings.intensity)  # :136
        s.light_dir[:] = [float(x) for x in self.lightSettings.direction]   # :140
        s.light_intensity = float(self.lightSettings.intensity)        # :139
        s.light_color[:] = [float(x) for x in self.lightSettings.color]     # :141
        t = self.traceSettings
        s.max_steps, s.ao_steps, s.max_bounces = int(t.maxRaySteps), int(t.aoSteps), int(t.maxReflections)
        s.shadows = 1 if t.shadows else 0
        s.traversal = int(t.traversal)
        s.flags = 4 if t.splitKernels else 0
        return s

    def denoiser_to_c(self) -> _capi.DenoiserSettings:
        d = self.denoiserSettings
        return _capi.DenoiserSettings(int(d.iterations), float(d.phiColor0), float(d.phiNormal0),
                                      float(d.phiPos0), float(d.stepWidth), int(d.mode))

    @staticmethod
    def primary_only(resolution=(1920, 1080), traversal=_capi.TRAVERSAL_AUTO) -> "VoxelRenderSettings":
        """BASELINE "primary rays only": ao_samples = 0 (ambient = 1), no shadow ray, no bounces, no FSR scale."""
        s = VoxelRenderSettings(targetResolution=tuple(resolution))
        s.fsrSetttings.enable = False
        s.denoiserSettings.enable = False
        s.occlusionSettings.numSamples = 0
        s.traceSettings.shadows = False
        s.traceSettings.maxReflections = 0
        s.traceSettings.traversal = traversal
        return s


# --------------------------------------------------------------------------------------------------
# camera (camera_controller.cpp:15-28)
# --------------------------------------------------------------------------------------------------

def _f32(x):
    return np.float32(x)


def _normalize(v):
    v = np.asarray(v, dtype=np.float32)
    n = np.sqrt(np.float32(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]))
    return (v / n).astype(np.float32)


class CameraController:
    def __init__(self, position=(8.0, 8.0, -50.0), yaw=90.0, pitch=0.0,
                 focalLength=1.0 / math.tan(math.radians(55.0 / 2))):       # voxel_renderer.cpp:20
        self.position = np.asarray(position, dtype=np.float32)
        self.yaw = float(yaw)
        self.pitch = float(pitch)
        self.focalLength = float(focalLength)
        self.updateDirectionVectors()

    def updateDirectionVectors(self):                                       # :15-28
        worldUp = np.array([0.0, -1.0, 0.0], dtype=np.float32)
        yaw, pitch = _f32(math.radians(self.yaw)), _f32(math.radians(self.pitch))
        nd = np.array([np.cos(yaw) * np.cos(pitch), np.sin(pitch), np.sin(yaw) * np.cos(pitch)], dtype=np.float32)
        self.normalDir = _normalize(nd)
        self.right = _normalize(np.cross(self.normalDir, worldUp).astype(np.float32))
        self.up = _normalize(np.cross(self.right, self.normalDir).astype(np.float32))
        self.direction = (self.normalDir * _f32(self.focalLength)).astype(np.float32)

    def update(self, delta: float, forward=0.0, strafe=0.0):                # :30-44 (keys -> scripted axes)
        cameraSpeed = _f32(50.0)
        self.position = (self.position + cameraSpeed * self.normalDir * _f32(delta) * _f32(forward)
                         + self.right * cameraSpeed * _f32(delta) * _f32(strafe)).astype(np.float32)
        self.updateDirectionVectors()

    def mouse(self, offsetX: float, offsetY: float):                        # :46-68 (right button held)
        self.yaw -= float(_f32(offsetX))
        self.pitch = float(min(max(_f32(self.pitch) - _f32(offsetY), _f32(-90.0)), _f32(90.0)))
        self.updateDirectionVectors()


@dataclass
class CameraKey:
    """One scripted input sample: what the keyboard / mouse callbacks of camera_controller.cpp:30-68 would have seen
    during `frames` consecutive frames (W/S -> forward +-1, D/A -> strafe +-1, cursor motion in pixels per frame)."""
    frames: int = 1
    forward: float = 0.0
    strafe: float = 0.0
    mouseX: float = 0.0
    mouseY: float = 0.0


def camera_path(camera: CameraController, keys, delta: float = 1.0 / 60.0):
    """Scripted fly-through: replays `keys` through CameraController.update / mouse and yields the controller after every
    frame (the same object, mutated), so a benchmark can render an animated sequence without a window."""
    for k in keys:
        for _ in range(int(k.frames)):
            if k.mouseX or k.mouseY:
                camera.mouse(k.mouseX, k.mouseY)
            camera.update(delta, k.forward, k.strafe)
            yield camera


# --------------------------------------------------------------------------------------------------
# engine / scene
# --------------------------------------------------------------------------------------------------

def _torch():
    import torch
    return torch


def _zeros(shape, dtype: str, device):
    torch = _torch()
    return torch.zeros(tuple(shape), dtype=getattr(torch, dtype), device=device)


def _ensure(tensor, shape, dtype: str, device):
    """`tensor` where it has `shape`; else a new one of zeros (a stage's image is recreated when its size changes)."""
    return tensor if tensor is not None and tuple(tensor.shape) == tuple(shape) else _zeros(shape, dtype, device)


def _ref(struct):
    """byref of a ctypes struct, NULL for None."""
    return C.byref(struct) if struct is not None else None


class Engine:
    """Device + stream holder (Engine::init, engine.cpp:14).  Work is enqueued on torch's current
    stream for the device so that torch ops (and RCCL collectives) order with the kernels."""

    def __init__(self, device: int = 0, use_torch_stream: bool = True):
        l = lib()
        self.device = int(device)
        torch = _torch()
        try:
            torch.cuda.init()                    # torch's HIP runtime first (see _capi.lib)
        except Exception:
            pass                                 # no GPU: vrt_ctx_create below reports it (VRT_ERR_NO_DEVICE, no CPU fallback)
        self._ctx = C.c_void_p()
        check(l.vrt_ctx_create(self.device, C.byref(self._ctx)))
        self.torch_device = torch.device("cuda", self.device)      # where the stages allocate their images
        if use_torch_stream:
            stream = torch.cuda.current_stream(self.torch_device)
            check(l.vrt_ctx_set_stream(self._ctx, C.c_void_p(stream.cuda_stream)))
        # use_torch_stream=False: the context keeps its own non-blocking stream (a second frame in flight); torch
        # allocations and fills on torch's stream must then be synchronised by the caller before the first use

    @property
    def ctx(self):
        if not self._ctx:
            raise RuntimeError("Engine was destroyed")
        return self._ctx

    def device_info(self):
        name = C.create_string_buffer(256)
        cus = C.c_int()
        check(lib().vrt_device_info(self.ctx, name, 256, C.byref(cus)))
        return name.value.decode(), cus.value

    def synchronize(self):
        check(lib().vrt_ctx_synchronize(self.ctx))

    def set_timing(self, enabled: bool):
        """Per-call HIP event recording inside the library (vrt_last_timings); off for throughput runs."""
        check(lib().vrt_ctx_set_timing(self.ctx, 1 if enabled else 0))

    def set_option(self, name: str, value) -> None:
        """Development switch of this context (include/vrt.h vrt_ctx_set_option): speed only, never a result."""
        check(lib().vrt_ctx_set_option(self.ctx, name.encode(), int(value)))

    def option(self, name: str) -> int:
        v = C.c_int32()
        check(lib().vrt_ctx_get_option(self.ctx, name.encode(), C.byref(v)))
        return int(v.value)

    def options(self, **kv):
        """with engine.options(tile_tags=0, sky_fast=0, sky_span=0): ...  -- the switches are put back on exit."""
        eng = self

        class _Scope:
            def __enter__(self_):
                self_.old = {k: eng.option(k) for k in kv}
                for k, v in kv.items():
                    eng.set_option(k, v)
                return eng

            def __exit__(self_, *a):
                for k, v in self_.old.items():
                    eng.set_option(k, v)
        return _Scope()

    def last_timings(self):
        a, b, c = C.c_float(), C.c_float(), C.c_float()
        check(lib().vrt_last_timings(self.ctx, C.byref(a), C.byref(b), C.byref(c)))
        return {"primary_ms": a.value, "geometry_ms": b.value, "denoise_ms": c.value}

    def destroy(self):
        if self._ctx:
            lib().vrt_ctx_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def materials_from_numpy(pal: np.ndarray):
    """pal: (256, 5) float32 [r, g, b, a, metallic] already linear -> ctypes Material[256]."""
    arr = (_capi.Material * 256)()
    pal = np.asarray(pal, dtype=np.float32)
    for i in range(256):
        arr[i].diffuse[:] = [float(x) for x in pal[i, :4]]
        arr[i].metallic = float(pal[i, 4])
    return arr


def materials_to_numpy(arr) -> np.ndarray:
    out = np.zeros((256, 5), dtype=np.float32)
    for i in range(256):
        out[i, :4] = list(arr[i].diffuse)
        out[i, 4] = arr[i].metallic
    return out


class VoxelScene:
    """VoxelScene(engine, filename, skyboxFilename) (voxel_scene.cpp:33).  `skyboxFilename` may be an
    (h, w, 4) float32 array (decoders for .hdr are a later-round item); None keeps the 1x1 white default.
    Raises RuntimeError with the reference's messages on load failures."""

    def __init__(self, engine: Engine, filename: Optional[str] = None, skyboxFilename=None, *, _handle=None):
        self.engine = engine
        self._h = C.c_void_p()
        if _handle is not None:
            self._h = _handle
        else:
            if filename is None:
                raise ValueError("VoxelScene needs a filename (or use VoxelScene.from_dense / from_memory)")
            rc = lib().vrt_scene_load_vox_file(engine.ctx, str(filename).encode(), C.byref(self._h))
            self._raise(rc)
        self._update_dims()
        if skyboxFilename is not None:
            self.set_sky(skyboxFilename)

    @staticmethod
    def _raise(rc):
        if rc != _capi.VRT_OK:
            msg = lib().vrt_last_error().decode()
            if rc in (2, 3, 4):
                raise RuntimeError(msg)          # reference: std::runtime_error, voxel_scene.cpp:42,46,50
            raise _capi.VrtError(rc, msg)

    @classmethod
    def from_memory(cls, engine: Engine, buf: bytes, sky=None):
        h = C.c_void_p()
        b = (C.c_uint8 * len(buf)).from_buffer_copy(buf)
        cls._raise(lib().vrt_scene_load_vox_mem(engine.ctx, b, len(buf), C.byref(h)))
        return cls(engine, skyboxFilename=sky, _handle=h)

    @classmethod
    def from_dense(cls, engine: Engine, voxels: np.ndarray, palette: np.ndarray, sky=None, noise=None):
        """voxels: uint8 array indexed [z, y, x] (C order == x + y*W + z*W*H); palette: (256,5) float32."""
        v = np.ascontiguousarray(voxels, dtype=np.uint8)
        D, H, W = v.shape
        h = C.c_void_p()
        cls._raise(lib().vrt_scene_from_dense(engine.ctx, v.ctypes.data_as(C.c_void_p), W, H, D,
                                              materials_from_numpy(palette), C.byref(h)))
        s = cls(engine, skyboxFilename=sky, _handle=h)
        if noise is not None:
            s.set_blue_noise(noise)
        return s

    @classmethod
    def from_bricks(cls, engine: Engine, grid: np.ndarray, pool: np.ndarray, palette: np.ndarray, sky=None, noise=None):
        """The volume in 8^3 bricks (vrt_scene_from_bricks): grid uint32 [nbz, nby, nbx] (0 = empty, else 1 + index into pool),
        pool uint8 [n, 8, 8, 8] indexed [z, y, x] within the brick.  Renders like from_dense of the same content."""
        g = np.ascontiguousarray(grid, dtype=np.uint32)
        p = np.ascontiguousarray(pool, dtype=np.uint8).reshape(-1, 512)
        nbz, nby, nbx = g.shape
        h = C.c_void_p()
        cls._raise(lib().vrt_scene_from_bricks(engine.ctx, g.ctypes.data_as(C.c_void_p), nbx, nby, nbz,
                                               p.ctypes.data_as(C.c_void_p) if p.size else None, p.shape[0],
                                               materials_from_numpy(palette), C.byref(h)))
        s = cls(engine, skyboxFilename=sky, _handle=h)
        if noise is not None:
            s.set_blue_noise(noise)
        return s

    def trim(self) -> None:
        """Drop the diagnostic copy of the clearance fields a launch with count planes built (vrt_scene_trim)."""
        check(lib().vrt_scene_trim(self.engine.ctx, self._h))

    def reserve_bricks(self, capacity: int) -> None:
        """Make a brick scene editable, with room for `capacity` bricks in its pool (vrt_scene_reserve_bricks); again with a larger
        capacity to grow.  What the scene renders does not change."""
        if not 0 <= int(capacity) <= 0xFFFFFFFF:
            raise ValueError("VoxelScene.reserve_bricks: capacity outside 0..2^32-1")
        self._raise(lib().vrt_scene_reserve_bricks(self.engine.ctx, self.handle, int(capacity)))

    def edit(self, lo, ids: np.ndarray) -> None:
        """Rewrite a box of a dense scene, or of a brick scene after reserve_bricks (vrt_scene_edit_box).  lo: (x, y, z) of its low corner; ids: uint8 array indexed [z, y, x]
        like from_dense's voxels (anything else is converted the same way), whose shape is the box.  Every later launch renders as
        on a scene newly built from the edited volume."""
        v = np.ascontiguousarray(ids, dtype=np.uint8)
        if v.ndim != 3:
            raise ValueError("VoxelScene.edit: ids must be indexed [z, y, x]")
        d, h, w = v.shape
        self._raise(lib().vrt_scene_edit_box(self.engine.ctx, self.handle, (C.c_int32 * 3)(*[int(t) for t in lo]), (C.c_uint32 * 3)(w, h, d),
                                             v.ctypes.data_as(C.c_void_p)))

    def fill(self, lo, size, id: int) -> None:
        """One id for the whole box lo .. lo + size, both (x, y, z) (vrt_scene_fill_box): 0 carves, non-zero fills."""
        if any(int(t) < 0 for t in size) or not 0 <= int(id) <= 255:
            raise ValueError("VoxelScene.fill: negative size or id outside 0..255")
        self._raise(lib().vrt_scene_fill_box(self.engine.ctx, self.handle, (C.c_int32 * 3)(*[int(t) for t in lo]),
                                             (C.c_uint32 * 3)(*[int(t) for t in size]), int(id)))

    # ---- brushes and stamps (vrt_scene_brush, vrt_scene_stamp; csrc/vrt_brush.h) ------------------------------------------
    BRUSH_SHAPES = {"box": _capi.BRUSH_BOX, "ellipsoid": _capi.BRUSH_ELLIPSOID, "capsule": _capi.BRUSH_CAPSULE}
    BRUSH_MODES = {"set": _capi.BRUSH_SET, "paint": _capi.BRUSH_PAINT, "add": _capi.BRUSH_ADD, "replace": _capi.BRUSH_REPLACE}

    @staticmethod
    def _half_voxels(v, what):
        """voxel units -> half voxels; only multiples of 0.5 have one"""
        out = []
        for t in np.atleast_1d(np.asarray(v, dtype=np.float64)).tolist():
            h = 2.0 * t
            if not (np.isfinite(h) and h == int(h) and abs(h) < 2 ** 31):
                raise ValueError(f"VoxelScene: {what} = {t} is not a multiple of 0.5 voxels")
            out.append(int(h))
        return out

    @staticmethod
    def _brush_result(res):
        return int(res.changed), tuple(int(t) for t in res.lo), tuple(int(t) for t in res.size)

    def brush(self, shape, mode, p, id: int = 0, match: int = 0):
        """One brush (vrt_scene_brush).  shape: "box" | "ellipsoid" | "capsule" (or its number), mode: "set" | "paint" | "add" |
        "replace", p: the shape's integer parameters as include/vrt.h lays them out (positions of ellipsoids and capsules in HALF
        voxels).  Returns (changed, lo, size): how many voxels changed and their tight box, zeros when none did."""
        sh = self.BRUSH_SHAPES[shape] if isinstance(shape, str) else int(shape)
        md = self.BRUSH_MODES[mode] if isinstance(mode, str) else int(mode)
        p = [int(t) for t in p]
        if len(p) > 9 or any(not -2 ** 31 <= t < 2 ** 31 for t in p) or not 0 <= int(id) <= 255 or not 0 <= int(match) <= 255:
            raise ValueError("VoxelScene.brush: at most nine int32 parameters, ids in 0..255")
        b = _capi.Brush(shape=sh, mode=md, id=int(id), match=int(match))
        b.p[:len(p)] = p
        res = _capi.BrushResult()
        self._raise(lib().vrt_scene_brush(self.engine.ctx, self.handle, C.byref(b), C.byref(res)))
        return self._brush_result(res)

    def box(self, lo, size, id: int, mode="set", match: int = 0):
        """A box of voxels lo .. lo + size (integers; lo may be negative, what lies outside the volume is clipped)."""
        if any(int(t) != t for t in list(lo) + list(size)):
            raise ValueError("VoxelScene.box: lo and size are whole voxels")
        return self.brush("box", mode, [int(t) for t in lo] + [int(t) for t in size], id, match)

    def ellipsoid(self, center, radii, id: int, mode="set", match: int = 0):
        """An ellipsoid; center and radii in voxel units, multiples of 0.5 (voxel (x, y, z) has its centre at (x+.5, y+.5, z+.5))."""
        return self.brush("ellipsoid", mode, self._half_voxels(center, "center") + self._half_voxels(radii, "radius"), id, match)

    def sphere(self, center, radius, id: int, mode="set", match: int = 0):
        return self.ellipsoid(center, (radius, radius, radius), id, mode, match)

    def capsule(self, a, b, radius, id: int, mode="set", match: int = 0):
        """Every voxel whose centre lies within `radius` of the segment a .. b (voxel units, multiples of 0.5): a dragged sphere."""
        return self.brush("capsule", mode, self._half_voxels(a, "a") + self._half_voxels(b, "b") + self._half_voxels(radius, "radius"), id, match)

    def stamp(self, dst_lo, src: "VoxelScene", src_lo, size, orient: int = 0, skip_empty: bool = False):
        """Paste the box src_lo .. src_lo + size of src (which may be this scene) at dst_lo, oriented by orient = perm | flips << 3
        (vrt_scene_stamp).  Returns (changed, lo, size) like brush."""
        if any(int(t) < 0 for t in size) or not 0 <= int(orient) <= 0xFFFFFFFF:
            raise ValueError("VoxelScene.stamp: negative size or orientation")
        res = _capi.BrushResult()
        self._raise(lib().vrt_scene_stamp(self.engine.ctx, self.handle, (C.c_int32 * 3)(*[int(t) for t in dst_lo]), src.handle,
                                          (C.c_int32 * 3)(*[int(t) for t in src_lo]), (C.c_uint32 * 3)(*[int(t) for t in size]), int(orient),
                                          _capi.STAMP_SKIP_EMPTY if skip_empty else 0, C.byref(res)))
        return self._brush_result(res)

    # ---- flood fills (vrt_scene_flood; csrc/vrt_flood.h) ---------------------------------------------------------------------
    FLOOD_MATCHES = {"same": _capi.FLOOD_SAME, "solid": _capi.FLOOD_SOLID}

    def _flood(self, seed, id, match, connectivity, bounds, flags):
        mt = self.FLOOD_MATCHES[match] if isinstance(match, str) else int(match)
        lo, size = ((0, 0, 0), (self.width, self.height, self.depth)) if bounds is None else bounds
        if any(int(t) < 0 for t in size) or not 0 <= int(id) <= 255:
            raise ValueError("VoxelScene.flood: negative size or id outside 0..255")
        f = _capi.Flood(match=mt, connectivity=int(connectivity), flags=flags, id=int(id))
        f.seed[:], f.lo[:], f.size[:] = [int(t) for t in seed], [int(t) for t in lo], [int(t) for t in size]
        res = _capi.FloodResult()
        self._raise(lib().vrt_scene_flood(self.engine.ctx, self.handle, C.byref(f), C.byref(res)))
        return res

    def flood(self, seed, id: int, match="same", connectivity: int = 6, bounds=None):
        """Every voxel connected to `seed` becomes `id` (vrt_scene_flood).  match: "same" (voxels with the seed's id, 0 included:
        the cavity fill) | "solid" (non-empty voxels); connectivity: 6 (faces) | 26 (faces, edges, corners); bounds: (lo, size)
        the search stays in, None = the whole volume (no side of it inside the volume above 512).  Returns a dict: region (its
        voxel count), region_lo, region_size, seed_id, and changed, lo, size as brush returns them."""
        res = self._flood(seed, id, match, connectivity, bounds, 0)
        return {"region": int(res.region), "region_lo": tuple(int(t) for t in res.region_lo), "region_size": tuple(int(t) for t in res.region_size),
                "seed_id": int(res.seed_id), "changed": int(res.edit.changed), "lo": tuple(int(t) for t in res.edit.lo),
                "size": tuple(int(t) for t in res.edit.size)}

    def region(self, seed, match="same", connectivity: int = 6, bounds=None):
        """How large the thing at `seed` is: (count, lo, size) of the region flood would rewrite; nothing is written
        (VRT_FLOOD_MEASURE).  Works on every scene, brick scenes that were never reserved included."""
        res = self._flood(seed, 0, match, connectivity, bounds, _capi.FLOOD_MEASURE)
        return int(res.region), tuple(int(t) for t in res.region_lo), tuple(int(t) for t in res.region_size)

    def flood_rounds(self) -> int:
        """(diagnostics) rounds of the tile kernel the latest flood of this scene ran"""
        n = C.c_uint32()
        check(lib().vrt_debug_flood_rounds(self.handle, C.byref(n)))
        return int(n.value)

    # ---- mesh voxelization (vrt_scene_voxelize; csrc/vrt_voxelize.h) ------------------------------------------------------
    VOXELIZE_FILLS = {"surface": _capi.VOXELIZE_SURFACE, "solid": _capi.VOXELIZE_SOLID, "both": _capi.VOXELIZE_SURFACE | _capi.VOXELIZE_SOLID}

    def voxelize(self, vertices, triangles, id: int, mode="set", fill="surface", bounds=None, match: int = 0):
        """A triangle mesh composed into the scene (vrt_scene_voxelize).  vertices: integers [nv][3] in SIXTEENTHS of a voxel
        (mesh_units converts floats in voxels); triangles: [nt][3] indices.  fill: "surface" (every voxel a triangle touches) |
        "solid" (every voxel whose centre is inside the mesh, parity along +x) | "both"; mode as brush; bounds: (lo, size) in
        voxels that may change, None = the mesh's own voxel bounds (no side of them inside the volume above 512).  Returns a dict:
        covered (voxels of the bounds the mesh covers), and changed, lo, size as brush returns them."""
        v = np.ascontiguousarray(np.asarray(vertices), np.int64).reshape(-1, 3)
        t = np.ascontiguousarray(np.asarray(triangles), np.int64).reshape(-1, 3)
        if v.size and (v.min() < -2 ** 31 or v.max() >= 2 ** 31) or t.size and (t.min() < 0 or t.max() >= 2 ** 32):
            raise ValueError("VoxelScene.voxelize: vertices are int32, indices uint32")
        if not 0 <= int(id) <= 255 or not 0 <= int(match) <= 255:
            raise ValueError("VoxelScene.voxelize: ids in 0..255")
        v32, t32 = np.ascontiguousarray(v, np.int32), np.ascontiguousarray(t, np.uint32)
        md = self.BRUSH_MODES[mode] if isinstance(mode, str) else int(mode)
        fl = self.VOXELIZE_FILLS[fill] if isinstance(fill, str) else int(fill)
        lo, size = mesh_voxel_bounds(v32) if bounds is None else bounds
        if any(int(s) < 0 for s in size):
            raise ValueError("VoxelScene.voxelize: negative size")
        job = _capi.Voxelize(mode=md, fill=fl, id=int(id), match=int(match))
        job.lo[:], job.size[:] = [int(s) for s in lo], [int(s) for s in size]
        res = _capi.VoxelizeResult()
        self._raise(lib().vrt_scene_voxelize(self.engine.ctx, self.handle, v32.ctypes.data if v32.size else None, v32.shape[0],
                                             t32.ctypes.data if t32.size else None, t32.shape[0], C.byref(job), C.byref(res)))
        return {"covered": int(res.covered), "changed": int(res.edit.changed), "lo": tuple(int(s) for s in res.edit.lo),
                "size": tuple(int(s) for s in res.edit.size)}

    def voxelize_item_rows(self, rows: int):
        """(diagnostics) rows per work item of this scene's voxelizations from now on; 0: the default"""
        check(lib().vrt_debug_voxelize_item_rows(self.handle, int(rows)))

    def voxelize_items(self) -> int:
        """(diagnostics) work items the latest voxelization of this scene launched"""
        n = C.c_uint32()
        check(lib().vrt_debug_voxelize_items(self.handle, C.byref(n)))
        return int(n.value)

    # ---- morphology (vrt_scene_morph; csrc/vrt_morph.h) ----------------------------------------------------------------------
    MORPH_OPS = {"dilate": _capi.MORPH_DILATE, "erode": _capi.MORPH_ERODE, "open": _capi.MORPH_OPEN, "close": _capi.MORPH_CLOSE,
                 "hollow": _capi.MORPH_HOLLOW}

    def morph(self, op, radius: int, connectivity: int = 6, id: int = 0, bounds=None, border_solid: bool = False, measure: bool = False):
        """Grow, shrink, open, close or hollow the scene's solid (vrt_scene_morph).  op: "dilate" | "erode" | "open" | "close" |
        "hollow" (or its number); radius 1..8; connectivity 6 (distance in L1) | 26 (L-infinity); id: what an added voxel becomes
        (dilate and close need one; no voxel is ever recoloured); bounds: (lo, size) that may change, None = the whole volume (no
        side of them inside the volume above 512); border_solid: the cells outside the volume count as solid; measure: write
        nothing.  Returns a dict: added, removed, and changed, lo, size as brush returns them (zeros under measure)."""
        o = self.MORPH_OPS[op] if isinstance(op, str) else int(op)
        lo, size = ((0, 0, 0), (self.width, self.height, self.depth)) if bounds is None else bounds
        if any(int(t) < 0 for t in size) or not 0 <= int(id) <= 255:
            raise ValueError("VoxelScene.morph: negative size or id outside 0..255")
        m = _capi.Morph(op=o, connectivity=int(connectivity), radius=int(radius), id=int(id),
                        flags=(_capi.MORPH_BORDER_SOLID if border_solid else 0) | (_capi.MORPH_MEASURE if measure else 0))
        m.lo[:], m.size[:] = [int(t) for t in lo], [int(t) for t in size]
        res = _capi.MorphResult()
        self._raise(lib().vrt_scene_morph(self.engine.ctx, self.handle, C.byref(m), C.byref(res)))
        return {"added": int(res.added), "removed": int(res.removed), "changed": int(res.edit.changed), "lo": tuple(int(t) for t in res.edit.lo),
                "size": tuple(int(t) for t in res.edit.size)}

    def dilate(self, radius: int, id: int, connectivity: int = 6, **kw):
        """Every empty voxel within `radius` of a solid one becomes `id`."""
        return self.morph("dilate", radius, connectivity, id, **kw)

    def erode(self, radius: int, connectivity: int = 6, **kw):
        """Every solid voxel within `radius` of an empty one becomes empty."""
        return self.morph("erode", radius, connectivity, 0, **kw)

    def open(self, radius: int, connectivity: int = 6, **kw):
        """Erode, then dilate what is left back: specks and spurs thinner than the ball go, nothing is added."""
        return self.morph("open", radius, connectivity, 0, **kw)

    def close(self, radius: int, id: int, connectivity: int = 6, **kw):
        """Dilate, then erode back: pinholes and gaps narrower than the ball become `id`, nothing is removed."""
        return self.morph("close", radius, connectivity, id, **kw)

    def hollow(self, radius: int = 1, connectivity: int = 6, **kw):
        """Keep a shell of thickness `radius` of every solid; the interior becomes empty."""
        return self.morph("hollow", radius, connectivity, 0, **kw)

    # ---- connected components (vrt_scene_components, vrt_scene_filter_components; csrc/vrt_components.h) ------------------
    COMP_MATCHES = {"solid": _capi.COMP_SOLID, "same": _capi.COMP_SAME, "empty": _capi.COMP_EMPTY}
    COMPONENT_DTYPE = np.dtype([("root", np.int32, 3), ("id", np.uint32), ("voxels", np.uint64), ("lo", np.int32, 3), ("size", np.uint32, 3),
                                ("faces", np.uint32), ("reserved", np.uint32)])

    def _components(self, match, connectivity, bounds):
        mt = self.COMP_MATCHES[match] if isinstance(match, str) else int(match)
        lo, size = ((0, 0, 0), (self.width, self.height, self.depth)) if bounds is None else bounds
        if any(int(t) < 0 for t in size):
            raise ValueError("VoxelScene.components: negative size")
        q = _capi.Components(match=mt, connectivity=int(connectivity), flags=0)
        q.lo[:], q.size[:] = [int(t) for t in lo], [int(t) for t in size]
        return q

    def components(self, match="solid", connectivity: int = 6, bounds=None):
        """Every connected component of the bounds at once (vrt_scene_components).  match: "solid" (non-empty voxels, whatever their
        ids) | "same" (non-empty voxels of one id) | "empty" (the cavities and the outer air); connectivity: 6 | 26; bounds: (lo,
        size), None = the whole volume (no side of them inside the volume above 512).  Returns (records, result): a structured
        array (COMPONENT_DTYPE: root, id, voxels, lo, size, faces) in component order -- ascending root -- and a dict: components,
        voxels, largest.  Nothing is written; works on every scene."""
        q = self._components(match, connectivity, bounds)
        res = _capi.ComponentsResult()
        self._raise(lib().vrt_scene_components(self.engine.ctx, self.handle, C.byref(q), None, 0, C.byref(res)))
        rec = np.zeros(int(res.components), dtype=self.COMPONENT_DTYPE)
        if rec.size:
            self._raise(lib().vrt_scene_components(self.engine.ctx, self.handle, C.byref(q), rec.ctypes.data_as(C.c_void_p), rec.size, C.byref(res)))
            assert int(res.components) == rec.size
        return rec, {"components": int(res.components), "voxels": int(res.voxels), "largest": int(res.largest)}

    def labels(self, box=None) -> np.ndarray:
        """The labels of the scene's latest labelling (vrt_scene_component_labels): a uint32 array indexed [z, y, x], a voxel's
        component number, 0xFFFFFFFF where it does not pass.  box: (lo, size) inside that labelling's clipped bounds; None = the
        whole volume.  VrtError once anything has rewritten the scene since."""
        lo, size = ((0, 0, 0), (self.width, self.height, self.depth)) if box is None else box
        clo, csz = self._box(lo, size)
        out = np.empty((int(size[2]), int(size[1]), int(size[0])), dtype=np.uint32)
        self._raise(lib().vrt_scene_component_labels(self.engine.ctx, self.handle, clo, csz, out.ctypes.data_as(C.c_void_p)))
        return out

    def filter_components(self, id: int, match="solid", connectivity: int = 6, bounds=None, min_voxels: int = 0, max_voxels: int = 2 ** 64 - 1,
                          faces_all: int = 0, faces_none: int = 0, keep_largest: bool = False, measure: bool = False):
        """Every voxel of every selected component becomes `id` (vrt_scene_filter_components).  Selected: min_voxels <= voxels <=
        max_voxels, touching all the faces of the bounds in faces_all and none of those in faces_none (bit d: 0 = -x .. 5 = +z),
        and under keep_largest not the largest.  measure: write nothing.  Returns a dict: components and voxels selected, and
        changed, lo, size as brush returns them."""
        q = self._components(match, connectivity, bounds)
        if not 0 <= int(id) <= 255 or not 0 <= int(min_voxels) < 2 ** 64 or not 0 <= int(max_voxels) < 2 ** 64 or not 0 <= int(faces_all) < 2 ** 32 \
                or not 0 <= int(faces_none) < 2 ** 32:
            raise ValueError("VoxelScene.filter_components: id in 0..255, counts in 0..2^64-1, face masks in 0..2^32-1")
        f = _capi.ComponentFilter(min_voxels=int(min_voxels), max_voxels=int(max_voxels), faces_all=int(faces_all), faces_none=int(faces_none),
                                  flags=(_capi.COMP_KEEP_LARGEST if keep_largest else 0) | (_capi.COMP_MEASURE if measure else 0), id=int(id))
        res = _capi.FilterResult()
        self._raise(lib().vrt_scene_filter_components(self.engine.ctx, self.handle, C.byref(q), C.byref(f), C.byref(res)))
        return {"components": int(res.components), "voxels": int(res.voxels), "changed": int(res.edit.changed),
                "lo": tuple(int(t) for t in res.edit.lo), "size": tuple(int(t) for t in res.edit.size)}

    def despeckle(self, min_voxels: int, connectivity: int = 6, **kw):
        """Delete every solid component of fewer than min_voxels voxels."""
        if int(min_voxels) < 1:
            raise ValueError("VoxelScene.despeckle: min_voxels >= 1")
        return self.filter_components(0, "solid", connectivity, max_voxels=int(min_voxels) - 1, **kw)

    def fill_cavities(self, id: int, connectivity: int = 6, **kw):
        """Every region of air that touches no face of the bounds becomes `id`."""
        return self.filter_components(id, "empty", connectivity, faces_none=63, **kw)

    def keep_largest(self, connectivity: int = 6, **kw):
        """Delete every solid component but the largest."""
        return self.filter_components(0, "solid", connectivity, keep_largest=True, **kw)

    # ---- read-back (vrt_scene_read_box, vrt_scene_list_box, vrt_scene_save_vox_*) ---------------------------------------
    @staticmethod
    def _box(lo, size):
        if any(int(t) < 0 for t in size):
            raise ValueError("VoxelScene: negative box size")
        return (C.c_int32 * 3)(*[int(t) for t in lo]), (C.c_uint32 * 3)(*[int(t) for t in size])

    def read(self, lo, size) -> np.ndarray:
        """The voxel ids of the box lo .. lo + size, both (x, y, z) (vrt_scene_read_box): a uint8 array indexed [z, y, x], the
        shape `edit` takes.  Dense scenes and brick scenes alike; an empty brick reads as zeros."""
        clo, csz = self._box(lo, size)
        out = np.empty((int(size[2]), int(size[1]), int(size[0])), dtype=np.uint8)
        self._raise(lib().vrt_scene_read_box(self.engine.ctx, self.handle, clo, csz, out.ctypes.data_as(C.c_void_p)))
        return out

    def count(self, lo, size) -> int:
        """Non-empty voxels of a box with no side above 256 (vrt_scene_list_box without records)."""
        clo, csz = self._box(lo, size)
        n = C.c_uint64()
        self._raise(lib().vrt_scene_list_box(self.engine.ctx, self.handle, clo, csz, None, 0, C.byref(n)))
        return int(n.value)

    def voxels(self, lo, size) -> np.ndarray:
        """The non-empty voxels of a box with no side above 256 (vrt_scene_list_box): uint32 records
        (x - lo[0]) | (y - lo[1]) << 8 | (z - lo[2]) << 16 | id << 24, in ascending order of x + y * size[0] + z * size[0] * size[1]."""
        clo, csz = self._box(lo, size)
        n = C.c_uint64()
        out = np.empty(self.count(lo, size), dtype=np.uint32)
        self._raise(lib().vrt_scene_list_box(self.engine.ctx, self.handle, clo, csz, out.ctypes.data_as(C.c_void_p) if out.size else None,
                                             out.size, C.byref(n)))
        assert int(n.value) == out.size
        return out

    def to_vox_bytes(self) -> bytes:
        """The scene as a MagicaVoxel .vox file (vrt_scene_save_vox_mem).  A palette that did not come from bytes is quantised."""
        buf, n = C.c_void_p(), C.c_size_t()
        self._raise(lib().vrt_scene_save_vox_mem(self.engine.ctx, self.handle, C.byref(buf), C.byref(n)))
        data = C.string_at(buf, n.value)
        lib().vrt_host_free(buf)
        return data

    def save(self, path) -> None:
        """Write the scene as it stands to a .vox file (vrt_scene_save_vox_file)."""
        self._raise(lib().vrt_scene_save_vox_file(self.engine.ctx, self.handle, os.fsencode(path)))

    # ---- surface extraction (vrt_scene_list_faces, vrt_scene_save_obj_*; csrc/vrt_faces.h) ------------------------------------
    @staticmethod
    def _face_flags(runs, closed):
        return (_capi.FACES_RUNS if runs else 0) | (_capi.FACES_CLOSED if closed else 0)

    def face_count(self, lo, size, runs=True, closed=False) -> np.ndarray:
        """Records per direction (-x, +x, -y, +y, -z, +z) of a box with no side above 256 (vrt_scene_list_faces without records)."""
        clo, csz = self._box(lo, size)
        counts = (C.c_uint64 * 6)()
        self._raise(lib().vrt_scene_list_faces(self.engine.ctx, self.handle, clo, csz, self._face_flags(runs, closed), None, 0, counts))
        return np.array(counts[:], dtype=np.uint64)

    def faces(self, lo, size, runs=True, closed=False):
        """The exposed faces of a box with no side above 256 (vrt_scene_list_faces) -> (records, counts): uint64 records
        list-box word | (length - 1) << 32 | d << 40 in ascending d and, within a d, ascending order key; counts uint64 (6,).
        runs: faces of one id in a row along the run axis merge (up to 64); closed: every voxel outside the box is empty."""
        clo, csz = self._box(lo, size)
        flags = self._face_flags(runs, closed)
        counts = (C.c_uint64 * 6)()
        out = np.empty(int(self.face_count(lo, size, runs, closed).sum()), dtype=np.uint64)
        self._raise(lib().vrt_scene_list_faces(self.engine.ctx, self.handle, clo, csz, flags, out.ctypes.data_as(C.c_void_p) if out.size else None,
                                               out.size, counts))
        got = np.array(counts[:], dtype=np.uint64)
        assert int(got.sum()) == out.size
        return out, got

    def to_obj_bytes(self, mtl_name="scene.mtl", runs=True):
        """The scene's surface as (OBJ bytes, MTL bytes) (vrt_scene_save_obj_mem); the OBJ names its library mtl_name."""
        obj, mtl, nobj, nmtl = C.c_void_p(), C.c_void_p(), C.c_size_t(), C.c_size_t()
        self._raise(lib().vrt_scene_save_obj_mem(self.engine.ctx, self.handle, os.fsencode(mtl_name), self._face_flags(runs, False), C.byref(obj),
                                                 C.byref(nobj), C.byref(mtl), C.byref(nmtl)))
        data = C.string_at(obj, nobj.value), C.string_at(mtl, nmtl.value)
        lib().vrt_host_free(obj)
        lib().vrt_host_free(mtl)
        return data

    def save_obj(self, path, runs=True) -> None:
        """Write the scene's surface to a Wavefront OBJ and, beside it, its .mtl (vrt_scene_save_obj_file): quads in integer
        voxel coordinates, grouped by id; read_obj reads the file back into mesh units."""
        self._raise(lib().vrt_scene_save_obj_file(self.engine.ctx, self.handle, os.fsencode(path), self._face_flags(runs, False)))

    # ---- ray queries (vrt_trace_rays, vrt_occluded_rays, vrt_pick_pixels) ----------------------------------------------
    RAY_PLANES = {"material": (np.uint8, 1), "pos": (np.float32, 3), "voxel": (np.int32, 3), "normal": (np.int8, 3)}

    def _query_in(self, a, dtype, cols, what):
        """A query's input as a contiguous device tensor [n, cols]: torch device tensors as they are (no copy when they
        already are contiguous and of the dtype), anything else uploaded.  Returns (tensor, came_from_torch)."""
        torch = _torch()
        tdt = {np.float32: torch.float32, np.int32: torch.int32}[dtype]
        if isinstance(a, torch.Tensor):
            if a.device != self.engine.torch_device:
                raise ValueError(f"{what}: tensor on {a.device}, the engine is on {self.engine.torch_device}")
            t = a.to(tdt).contiguous()
            came = True
        else:
            t = torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(self.engine.torch_device)
            came = False
        if t.ndim != 2 or t.shape[1] != cols:
            raise ValueError(f"{what}: expected shape (n, {cols}), got {tuple(t.shape)}")
        return t, came

    def _query_out(self, n, planes):
        torch = _torch()
        tdt = {np.uint8: torch.uint8, np.float32: torch.float32, np.int32: torch.int32, np.int8: torch.int8}
        planes = tuple(planes)
        if not planes or any(p not in self.RAY_PLANES for p in planes):
            raise ValueError(f"planes: a non-empty subset of {tuple(self.RAY_PLANES)}")
        out = {}
        for p in planes:
            dt, k = self.RAY_PLANES[p]
            out[p] = torch.empty((n,) if k == 1 else (n, k), dtype=tdt[dt], device=self.engine.torch_device)
        hits = _capi.RayHits(**{p: C.c_void_p(t.data_ptr()) for p, t in out.items()})
        return out, hits

    def _query_result(self, out, came):
        if came:
            return out
        self.engine.synchronize()          # (the context may run on a stream of its own)
        return {k: v.cpu().numpy() for k, v in out.items()}

    def trace_rays(self, origins, dirs, max_steps=512, planes=("material", "pos", "voxel", "normal")):
        """Closest hit of n rays (vrt_trace_rays): origins, dirs (n, 3) float32 in volume coordinates, directions used as given.
        Returns {plane: array} for the planes asked for: material uint8 (n,), 0 = miss; pos float32 (n, 3); voxel int32 (n, 3);
        normal int8 (n, 3); a miss is 0 everywhere.  Torch device tensors go in and come out without a copy, on the engine's
        stream and without waiting for it; numpy arrays are uploaded and the results come back as numpy."""
        o, came_o = self._query_in(origins, np.float32, 3, "trace_rays: origins")
        d, came_d = self._query_in(dirs, np.float32, 3, "trace_rays: dirs")
        if o.shape[0] != d.shape[0]:
            raise ValueError("trace_rays: origins and dirs differ in length")
        n = int(o.shape[0])
        out, hits = self._query_out(n, planes)
        if n == 0:                                   # (an empty tensor has no address to hand over; the C call would launch nothing)
            return self._query_result(out, came_o and came_d)
        self._raise(lib().vrt_trace_rays(self.engine.ctx, self.handle, n, C.c_void_p(o.data_ptr()), C.c_void_p(d.data_ptr()),
                                         int(max_steps), C.byref(hits)))
        return self._query_result(out, came_o and came_d)

    def _query_tmax(self, t_max, n, what):
        """A segment query's limits as a contiguous device tensor [n] of float32 (a scalar serves every ray)."""
        torch = _torch()
        if isinstance(t_max, torch.Tensor):
            if t_max.device != self.engine.torch_device:
                raise ValueError(f"{what}: tensor on {t_max.device}, the engine is on {self.engine.torch_device}")
            t, came = t_max.to(torch.float32).contiguous(), True
        else:
            a = np.asarray(t_max, dtype=np.float32)
            t, came = torch.from_numpy(np.ascontiguousarray(np.full(n, a, np.float32) if a.ndim == 0 else a)).to(self.engine.torch_device), False
        if t.ndim != 1 or t.shape[0] != n:
            raise ValueError(f"{what}: expected shape ({n},), got {tuple(t.shape)}")
        return t, came

    def trace_segments(self, origins, dirs, t_max, max_steps=512, planes=("material", "pos", "voxel", "normal", "t")):
        """Closest hit of n rays within a distance limit per ray (vrt_trace_segments): trace_rays' arguments and planes, t_max (n,)
        float32 (or one number for all) and the plane "t" float32 (n,), the hit's parameter along the ray as given -- in units of
        dirs, so with origins A and dirs B - A, t = 1 is B.  A hit is kept iff t <= t_max; one that is not is a miss, 0 in every
        plane and in t.  NaN keeps nothing, +inf everything (the planes are then trace_rays')."""
        o, came_o = self._query_in(origins, np.float32, 3, "trace_segments: origins")
        d, came_d = self._query_in(dirs, np.float32, 3, "trace_segments: dirs")
        if o.shape[0] != d.shape[0]:
            raise ValueError("trace_segments: origins and dirs differ in length")
        n = int(o.shape[0])
        tm, came_t = self._query_tmax(t_max, n, "trace_segments: t_max")
        planes = tuple(planes)
        if not planes or any(p != "t" and p not in self.RAY_PLANES for p in planes):
            raise ValueError(f"planes: a non-empty subset of {tuple(self.RAY_PLANES) + ('t',)}")
        torch = _torch()
        rec = tuple(p for p in planes if p != "t")
        out, hits = self._query_out(n, rec) if rec else ({}, None)
        t = torch.empty((n,), dtype=torch.float32, device=self.engine.torch_device) if "t" in planes else None
        if t is not None:
            out["t"] = t
        came = came_o and came_d and came_t
        if n == 0:
            return self._query_result(out, came)
        self._raise(lib().vrt_trace_segments(self.engine.ctx, self.handle, n, C.c_void_p(o.data_ptr()), C.c_void_p(d.data_ptr()),
                                             C.c_void_p(tm.data_ptr()), int(max_steps), C.byref(hits) if hits is not None else None,
                                             C.c_void_p(t.data_ptr()) if t is not None else None))
        return self._query_result(out, came)

    def occluded(self, origins, dirs, max_steps=512, t_max=None):
        """Any hit (vrt_occluded_rays): uint8 (n,), 1 where the ray meets a voxel within max_steps.  t_max (n,) float32 or one
        number (vrt_occluded_segments): ... and no farther along the ray than t_max, in units of dirs (trace_segments)."""
        torch = _torch()
        o, came_o = self._query_in(origins, np.float32, 3, "occluded: origins")
        d, came_d = self._query_in(dirs, np.float32, 3, "occluded: dirs")
        if o.shape[0] != d.shape[0]:
            raise ValueError("occluded: origins and dirs differ in length")
        n = int(o.shape[0])
        came = came_o and came_d
        if t_max is not None:
            tm, came_t = self._query_tmax(t_max, n, "occluded: t_max")
            came = came and came_t
        occ = torch.empty((n,), dtype=torch.uint8, device=self.engine.torch_device)
        if n == 0:
            return self._query_result({"occluded": occ}, came)["occluded"]
        if t_max is not None:
            self._raise(lib().vrt_occluded_segments(self.engine.ctx, self.handle, n, C.c_void_p(o.data_ptr()), C.c_void_p(d.data_ptr()),
                                                    C.c_void_p(tm.data_ptr()), int(max_steps), C.c_void_p(occ.data_ptr())))
        else:
            self._raise(lib().vrt_occluded_rays(self.engine.ctx, self.handle, n, C.c_void_p(o.data_ptr()), C.c_void_p(d.data_ptr()),
                                                int(max_steps), C.c_void_p(occ.data_ptr())))
        return self._query_result({"occluded": occ}, came)["occluded"]

    def visible(self, a, b, max_steps=512):
        """Line of sight between point pairs: bool (n,), True where no voxel lies between a[i] and b[i] -- the segment from a to b
        as one ray with origin a, direction b - a (subtracted in float32) and t_max = 1 (vrt_occluded_segments), negated.  a, b:
        (n, 3) float32 in volume coordinates, numpy or torch as for trace_rays.  Inherited from the reference's boxIntersection:
        where a lies outside the volume the ray is advanced 0.1 * |b - a| voxels past the face it enters through before it
        looks at a voxel, so a voxel that close behind the face is not seen; a pair inside the volume has no such gap."""
        torch = _torch()
        if isinstance(a, torch.Tensor) != isinstance(b, torch.Tensor):
            raise ValueError("visible: a and b must both be torch tensors or both be host arrays")
        if isinstance(a, torch.Tensor):
            # (b - a and the limits are made on torch's current stream: an engine with a stream of its own leaves their ordering
            # to the caller, as for every tensor it is handed)
            ta, tb = a.to(torch.float32), b.to(torch.float32)
            if ta.shape != tb.shape:
                raise ValueError("visible: a and b differ in shape")
            one = torch.ones((int(ta.shape[0]),), dtype=torch.float32, device=ta.device)
            return self.occluded(ta, tb - ta, max_steps, t_max=one) == 0
        na, nb = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
        if na.shape != nb.shape:
            raise ValueError("visible: a and b differ in shape")
        return self.occluded(na, nb - na, max_steps, t_max=1.0) == 0

    def pick(self, push, xy, max_steps=512, planes=("material", "pos", "voxel", "normal")):
        """The voxels under n pixels (vrt_pick_pixels): xy (n, 2) int32 pixel coordinates, push the frame's push constants
        (make_push / VoxelRenderer.push_constants).  Record i is what a frame rendered with that push holds at pixel xy[i]; a
        pixel outside the screen is a miss.  Results as trace_rays returns them."""
        t, came = self._query_in(xy, np.int32, 2, "pick: xy")
        n = int(t.shape[0])
        out, hits = self._query_out(n, planes)
        if n == 0:
            return self._query_result(out, came)
        self._raise(lib().vrt_pick_pixels(self.engine.ctx, self.handle, C.byref(push), int(max_steps), n, C.c_void_p(t.data_ptr()),
                                          C.byref(hits)))
        return self._query_result(out, came)

    def debug_state(self, what: int) -> np.ndarray:
        """One of a scene's device structures as it lies in memory (vrt_debug_scene_state; _capi.STATE_*): uint8 for the voxels
        and the clearance fields, uint64 for the pyramid levels, uint32 for the occupied cells; of a brick scene uint64 for the
        packed entries, uint8 [slots, 512] for the pool and [slots, 8, 512] for the per-voxel clearances."""
        n = C.c_size_t()
        self._raise(lib().vrt_debug_scene_state(self.engine.ctx, self.handle, int(what), None, 0, C.byref(n)))
        dt = {_capi.STATE_OCC1: np.uint64, _capi.STATE_OCC2: np.uint64, _capi.STATE_OCC3: np.uint64, _capi.STATE_CELLS: np.uint32,
              _capi.STATE_BENTRY: np.uint64}.get(int(what), np.uint8)
        out = np.empty(n.value // np.dtype(dt).itemsize, dtype=dt)
        self._raise(lib().vrt_debug_scene_state(self.engine.ctx, self.handle, int(what), out.ctypes.data_as(C.c_void_p), out.nbytes, C.byref(n)))
        if int(what) == _capi.STATE_BPOOL:
            return out.reshape(-1, 512)
        if int(what) == _capi.STATE_BFINE:
            return out.reshape(-1, 8, 512)
        return out

    def memory_bytes(self) -> int:
        n = C.c_uint64()
        check(lib().vrt_scene_memory(self._h, C.byref(n)))
        return int(n.value)

    def _update_dims(self):
        d = (C.c_uint32 * 3)()
        check(lib().vrt_scene_info(self._h, d))
        self.width, self.height, self.depth = int(d[0]), int(d[1]), int(d[2])

    def set_sky(self, rgba):
        if isinstance(rgba, (str, bytes, os.PathLike)):       # Texture2D(skyboxPath, 4, RGBA32F): decode on the host
            rc = lib().vrt_scene_set_sky_file(self.engine.ctx, self._h, os.fsencode(rgba))
            if rc != _capi.VRT_OK:
                raise RuntimeError(lib().vrt_last_error().decode())      # "Could not load image <path>" (texture_2d.cpp:42)
            return
        self._set_sky_array(rgba)

    def _set_sky_array(self, rgba: np.ndarray):
        a = np.ascontiguousarray(rgba, dtype=np.float32)
        assert a.ndim == 3 and a.shape[2] == 4
        check(lib().vrt_scene_set_sky(self.engine.ctx, self._h, a.ctypes.data_as(C.c_void_p), a.shape[1], a.shape[0]))

    def set_blue_noise(self, rgba8):
        if isinstance(rgba8, (str, bytes, os.PathLike)):      # Texture2D("blue_noise_rgba.png", 4, RGBA8_UNORM)
            rc = lib().vrt_scene_set_blue_noise_file(self.engine.ctx, self._h, os.fsencode(rgba8))
            if rc != _capi.VRT_OK:
                raise RuntimeError(lib().vrt_last_error().decode())
            return
        self._set_noise_array(rgba8)

    def _set_noise_array(self, rgba8: np.ndarray):
        a = np.ascontiguousarray(rgba8, dtype=np.uint8)
        assert a.ndim == 3 and a.shape[2] == 4
        check(lib().vrt_scene_set_blue_noise(self.engine.ctx, self._h, a.ctypes.data_as(C.c_void_p), a.shape[1], a.shape[0]))

    def download(self):
        v = np.empty((self.depth, self.height, self.width), dtype=np.uint8)
        pal = (_capi.Material * 256)()
        check(lib().vrt_scene_download(self.engine.ctx, self._h, v.ctypes.data_as(C.c_void_p), pal))
        return v, materials_to_numpy(pal)

    @property
    def handle(self):
        if not self._h:
            raise RuntimeError("VoxelScene was destroyed")
        return self._h

    def destroy(self):
        if self._h:
            lib().vrt_scene_free(self.engine.ctx, self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def mesh_units(float_vertices) -> np.ndarray:
    """Positions in voxels -> the integers vrt_scene_voxelize takes (sixteenths of a voxel): np.rint(np.float32(v) * 16) as int32.
    The multiplication by 16 is exact in float32 (a power of two) and the rounding is to nearest, ties to even; this is the only
    place floating point enters a voxelization."""
    v = np.asarray(float_vertices, np.float32) * np.float32(_capi.VOXELIZE_UNIT)
    return np.rint(v).astype(np.int32).reshape(-1, 3)


def mesh_voxel_bounds(vertices):
    """(lo, size) of the voxels whose closed cube [16x, 16x+16]^3 a mesh's vertices (sixteenths of a voxel) can touch"""
    v = np.asarray(vertices, np.int64).reshape(-1, 3)
    if v.size == 0:
        return (0, 0, 0), (1, 1, 1)
    lo = [-((-int(v[:, a].min())) // 16) - 1 for a in range(3)]
    hi = [int(v[:, a].max()) // 16 for a in range(3)]
    return tuple(lo), tuple(hi[a] - lo[a] + 1 for a in range(3))


def read_obj(path):
    """A minimal Wavefront OBJ reader -> (vertices in mesh units [nv][3] int32, triangles [nt][3] uint32): `v` and `f` lines only,
    polygons as fans around their first corner, negative (relative) indices, everything after a `/` in a corner ignored.
    Coordinates are taken as voxels and converted by mesh_units."""
    verts, tris = [], []
    with open(path, "r") as f:
        for line in f:
            w = line.split("#", 1)[0].split()
            if not w:
                continue
            if w[0] == "v" and len(w) >= 4:
                verts.append([float(w[1]), float(w[2]), float(w[3])])
            elif w[0] == "f" and len(w) >= 4:
                idx = []
                for corner in w[1:]:
                    i = int(corner.split("/", 1)[0])
                    i = i - 1 if i > 0 else len(verts) + i
                    if not 0 <= i < len(verts):
                        raise ValueError(f"read_obj: {path}: face corner {corner} names no vertex read so far")
                    idx.append(i)
                tris.extend([idx[0], idx[k], idx[k + 1]] for k in range(1, len(idx) - 1))
    return mesh_units(np.asarray(verts, np.float32).reshape(-1, 3)), np.asarray(tris, np.uint32).reshape(-1, 3)


def faces_mesh(records, lo):
    """Records of VoxelScene.faces for a box at lo -> (vertices int32 (nv, 3) in mesh units, welded in order of first appearance,
    quads uint32 (n, 4), ids uint8 (n,)) (vrt_faces_mesh_host; host only).  A quad's corners start at its lowest corner and run
    counter-clockwise seen from the empty side."""
    r = np.ascontiguousarray(records, dtype=np.uint64).reshape(-1)
    v, q, i, nv = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64()
    clo = (C.c_int32 * 3)(*[int(t) for t in lo])
    VoxelScene._raise(lib().vrt_faces_mesh_host(r.ctypes.data_as(C.c_void_p) if r.size else None, r.size, clo, C.byref(v), C.byref(nv), C.byref(q), C.byref(i)))
    n = int(nv.value)
    verts = np.ctypeslib.as_array(C.cast(v, C.POINTER(C.c_int32)), shape=(max(n * 3, 1),))[:n * 3].copy().reshape(n, 3)
    quads = np.ctypeslib.as_array(C.cast(q, C.POINTER(C.c_uint32)), shape=(max(r.size * 4, 1),))[:r.size * 4].copy().reshape(r.size, 4)
    ids = np.ctypeslib.as_array(C.cast(i, C.POINTER(C.c_uint8)), shape=(max(r.size, 1),))[:r.size].copy()
    for p in (v, q, i):
        lib().vrt_host_free(p)
    return verts, quads, ids


def quads_to_triangles(quads) -> np.ndarray:
    """Quads (n, 4) as fans around their first corner -> triangles uint32 (2n, 3): (a, b, c), (a, c, d), the quad's orientation kept"""
    q = np.asarray(quads, np.uint32).reshape(-1, 4)
    return np.stack([q[:, [0, 1, 2]], q[:, [0, 2, 3]]], axis=1).reshape(-1, 3)


def faces_obj_host(records, lo, palette, mtl_name="scene.mtl"):
    """Records of a box at lo -> (OBJ bytes, MTL bytes) (vrt_faces_obj_host; host only): what VoxelScene.save_obj writes for a
    scene of one tile.  palette (256, 5) float32."""
    r = np.ascontiguousarray(records, dtype=np.uint64).reshape(-1)
    obj, mtl, nobj, nmtl = C.c_void_p(), C.c_void_p(), C.c_size_t(), C.c_size_t()
    clo = (C.c_int32 * 3)(*[int(t) for t in lo])
    VoxelScene._raise(lib().vrt_faces_obj_host(r.ctypes.data_as(C.c_void_p) if r.size else None, r.size, clo, materials_from_numpy(palette),
                                               os.fsencode(mtl_name), C.byref(obj), C.byref(nobj), C.byref(mtl), C.byref(nmtl)))
    data = C.string_at(obj, nobj.value), C.string_at(mtl, nmtl.value)
    lib().vrt_host_free(obj)
    lib().vrt_host_free(mtl)
    return data


def load_image(path):
    """Host-side decoder behind Texture2D (Radiance .hdr -> float32 RGBA, PNG -> uint8 RGBA)."""
    hdr, w, h, px = C.c_int(), C.c_uint32(), C.c_uint32(), C.c_void_p()
    rc = lib().vrt_image_load(os.fsencode(path), C.byref(hdr), C.byref(w), C.byref(h), C.byref(px))
    if rc != _capi.VRT_OK:
        raise RuntimeError(lib().vrt_last_error().decode())
    n = w.value * h.value * 4
    if hdr.value:
        a = np.ctypeslib.as_array(C.cast(px, C.POINTER(C.c_float)), shape=(n,)).copy().reshape(h.value, w.value, 4)
    else:
        a = np.ctypeslib.as_array(C.cast(px, C.POINTER(C.c_uint8)), shape=(n,)).copy().reshape(h.value, w.value, 4)
    lib().vrt_host_free(px)
    return a


def write_image(path, array):
    """PNG / PPM from uint8 RGBA (H,W,4); PFM from float32 (H,W,3|4)."""
    a = np.ascontiguousarray(array)
    p = os.fsencode(path)
    H, W = a.shape[:2]
    if a.dtype == np.uint8:
        fn = lib().vrt_image_write_ppm if str(path).lower().endswith(".ppm") else lib().vrt_image_write_png
        check(fn(p, a.ctypes.data_as(C.c_void_p), W, H))
    else:
        a = np.ascontiguousarray(a, dtype=np.float32)
        check(lib().vrt_image_write_pfm(p, a.ctypes.data_as(C.c_void_p), W, H, a.shape[2]))


def vox_flatten_host(buf: bytes):
    """Host-only .vox parse + flatten (no device): returns (voxels[z,y,x], palette(256,5), n_instances, dropped)."""
    dims = (C.c_uint32 * 3)()
    vox = C.c_void_p()
    pal = (_capi.Material * 256)()
    ninst, dropped = C.c_uint32(), C.c_uint64()
    b = (C.c_uint8 * len(buf)).from_buffer_copy(buf)
    rc = lib().vrt_vox_flatten_host(b, len(buf), dims, C.byref(vox), pal, C.byref(ninst), C.byref(dropped))
    VoxelScene._raise(rc)
    W, H, D = int(dims[0]), int(dims[1]), int(dims[2])
    arr = np.ctypeslib.as_array(C.cast(vox, C.POINTER(C.c_uint8)), shape=(D * H * W,)).copy().reshape(D, H, W)
    lib().vrt_host_free(vox)
    return arr, materials_to_numpy(pal), ninst.value, dropped.value


def vox_encode_host(voxels: np.ndarray, palette: np.ndarray) -> bytes:
    """Host-only .vox writer (no device; vrt_vox_encode_host): voxels uint8 [z, y, x], palette (256, 5) float32.  The inverse of
    vox_flatten_host for palettes that came from bytes; any other palette is quantised."""
    v = np.ascontiguousarray(voxels, dtype=np.uint8)
    if v.ndim != 3:
        raise ValueError("vox_encode_host: voxels must be indexed [z, y, x]")
    D, H, W = v.shape
    buf, n = C.c_void_p(), C.c_size_t()
    VoxelScene._raise(lib().vrt_vox_encode_host(v.ctypes.data_as(C.c_void_p), (C.c_uint32 * 3)(W, H, D), materials_from_numpy(palette),
                                                C.byref(buf), C.byref(n)))
    data = C.string_at(buf, n.value)
    lib().vrt_host_free(buf)
    return data


# --------------------------------------------------------------------------------------------------
# push constants (voxel_renderer.cpp:72-83)
# --------------------------------------------------------------------------------------------------

def make_push(camera: CameraController, scene_dims, resolution, frame=0, jitter=(0.0, 0.0)) -> _capi.Push:
    p = _capi.Push()
    p.screen_size[:] = [int(resolution[0]), int(resolution[1])]
    p.volume_bounds[:] = [int(scene_dims[0]), int(scene_dims[1]), int(scene_dims[2])]
    p.cam_pos[:] = [float(camera.position[0]), float(camera.position[1]), float(camera.position[2]), 1.0]
    p.cam_dir[:] = [float(camera.direction[0]), float(camera.direction[1]), float(camera.direction[2]), 0.0]
    p.cam_up[:] = [float(camera.up[0]), float(camera.up[1]), float(camera.up[2]), 0.0]
    p.cam_right[:] = [float(camera.right[0]), float(camera.right[1]), float(camera.right[2]), 0.0]
    p.frame = int(frame) & 0xFFFFFFFF
    p.camera_jitter[:] = [float(jitter[0]), float(jitter[1])]
    return p


class RayCamera:
    """A camera model whose rays vrt_camera_rays makes on the device (csrc/vrt_raygen.h defines the three models): the built-in
    pinhole with any field of view, an orthographic view, an equirectangular panorama -- as the two (W * H, 3) tensors that
    VoxelScene.trace_rays and VoxelScene.occluded take."""

    def __init__(self, model: int, camera: CameraController, tan_half: float = 1.0, half_width: float = 1.0):
        self.model, self.camera = int(model), camera
        self.tan_half, self.half_width = float(tan_half), float(half_width)

    @classmethod
    def perspective(cls, controller: CameraController, fov_deg: float = 90.0) -> "RayCamera":
        """main()'s pinhole with a horizontal field of view of fov_deg; 90 is the reference's camera bit for bit (tan_half = 1)."""
        return cls(_capi.CAMERA_PERSPECTIVE, controller, tan_half=float(np.float32(math.tan(math.radians(float(fov_deg)) / 2.0))))

    @classmethod
    def orthographic(cls, controller: CameraController, half_width: float) -> "RayCamera":
        """Parallel rays along the controller's direction; the view is 2 * half_width voxels wide."""
        return cls(_capi.CAMERA_ORTHOGRAPHIC, controller, half_width=half_width)

    @classmethod
    def panorama(cls, position) -> "RayCamera":
        """Equirectangular around `position`, the inverse of the sky's own mapping."""
        return cls(_capi.CAMERA_PANORAMA, CameraController(position=position))

    def to_c(self, resolution, jitter=(0.0, 0.0)) -> _capi.RayCamera:
        c = _capi.RayCamera()
        c.model = self.model
        c.basis = make_push(self.camera, (0, 0, 0), resolution, 0, jitter)
        c.tan_half, c.half_width = self.tan_half, self.half_width
        return c

    def rays(self, engine: "Engine", resolution, jitter=(0.0, 0.0), offset=(0.0, 0.0)):
        """(origins, dirs): two float32 device tensors (W * H, 3), ray py * W + px for pixel (px, py); the jitter, in pixels,
        applies to the perspective model only.  offset, in pixels and within one pixel, moves every sample from its pixel's
        centre under all three models (vrt_camera_rays_offset); (0, 0) is vrt_camera_rays.  Enqueued on the engine's stream, not
        waited for."""
        torch = _torch()
        W, H = int(resolution[0]), int(resolution[1])
        cam = self.to_c((W, H), jitter)
        o = torch.empty((max(W * H, 0), 3), dtype=torch.float32, device=engine.torch_device)
        d = torch.empty_like(o)
        if float(offset[0]) != 0.0 or float(offset[1]) != 0.0:
            off = (C.c_float * 2)(float(offset[0]), float(offset[1]))
            check(lib().vrt_camera_rays_offset(engine.ctx, C.byref(cam), W, H, off, C.c_void_p(o.data_ptr()), C.c_void_p(d.data_ptr())))
        else:
            check(lib().vrt_camera_rays(engine.ctx, C.byref(cam), W, H, C.c_void_p(o.data_ptr()), C.c_void_p(d.data_ptr())))
        return o, d


# --------------------------------------------------------------------------------------------------
# stages
# --------------------------------------------------------------------------------------------------

_PLANE_SPECS = {
    # name: (torch dtype name, trailing shape)
    "color8": ("uint8", (4,)), "depth": ("float32", ()), "motion": ("float32", (2,)), "mask8": ("uint8", ()),
    "position": ("float32", (4,)), "normal8": ("int8", (4,)),
    "color_f": ("float32", (3,)), "hit_id": ("uint8", ()), "hit_voxel": ("int16", (3,)), "hit_mask": ("uint8", ()),
    "steps_primary": ("int32", ()), "steps_total": ("int32", ()), "rays_total": ("int32", ()),
    "color8_strips": ("uint8", (4,)),      # (allocated at the full frame's size: the packed strips of a rank fill its first rows)
}
GBUFFER_PLANES = ("color8", "depth", "motion", "mask8", "position", "normal8")
DEBUG_PLANES = ("color_f", "hit_id", "hit_voxel", "hit_mask", "steps_primary", "steps_total", "rays_total")
# Planes whose presence changes which march a launch runs: the count planes select the clearance fields without open cells
# (the iterations of the reference's loop), hit_voxel the look-up loop that keeps mapPos.  A stage with debug planes renders
# them in a launch of their own, so that every other plane comes from the march a caller without debug planes gets.
DIAGNOSTIC_MARCH_PLANES = ("hit_voxel", "steps_primary", "steps_total")


class GeometryBuffer:
    """GeometryBuffer (geometry_stage.hpp:19-27): color, depth, motion, mask, normal, position (+ debug planes).
    Each plane is a torch tensor on the engine's device, shape (H, W, ...)."""

    def __init__(self, engine: Engine, W: int, H: int, planes=GBUFFER_PLANES):
        torch = _torch()
        self.W, self.H = int(W), int(H)
        self.planes = {}
        for n in planes:
            dt, tail = _PLANE_SPECS[n]
            self.planes[n] = torch.zeros((self.H, self.W) + tail, dtype=getattr(torch, dt), device=engine.torch_device)

    def __getattr__(self, n):
        alias = {"color": "color8", "mask": "mask8", "normal": "normal8"}
        planes = self.__dict__.get("planes", {})
        n2 = alias.get(n, n)
        if n2 in planes:
            return planes[n2]
        raise AttributeError(n)

    def to_c(self, only=None, without=()) -> _capi.Frame:
        f = _capi.Frame()
        for n in _capi.FRAME_PLANES:
            t = self.planes.get(n)
            if (only is not None and n not in only) or n in without:
                t = None
            setattr(f, n, t.data_ptr() if t is not None else None)
        return f

    def to_c_split(self):
        """[frame of the product march, frame of the diagnostic march or None] (DIAGNOSTIC_MARCH_PLANES)."""
        if not any(n in self.planes for n in DIAGNOSTIC_MARCH_PLANES):
            return [self.to_c(), None]
        return [self.to_c(without=DIAGNOSTIC_MARCH_PLANES), self.to_c(only=DIAGNOSTIC_MARCH_PLANES)]

    def numpy(self):
        return {n: t.cpu().numpy() for n, t in self.planes.items()}


def make_shard(rank=0, nranks=1, strip_rows=16):
    if nranks <= 1:
        return None
    return _capi.Shard(int(rank), int(nranks), int(strip_rows))


class GeometryStage:
    """GeometryStage(engine, settings, scene, noise) / record() (geometry_stage.cpp:14,106)."""

    def __init__(self, engine: Engine, settings: VoxelRenderSettings, scene: VoxelScene, noise=None,
                 debug_planes: bool = False):
        self.engine, self._settings, self._scene = engine, settings, scene
        if noise is not None:
            scene.set_blue_noise(noise)
        self._debug = debug_planes
        self._buffer = None

    def _targets(self):
        W, H = self._settings.renderResolution()
        if self._buffer is None or (self._buffer.W, self._buffer.H) != (W, H):     # RENDER_RESIZE recreation
            planes = GBUFFER_PLANES + (DEBUG_PLANES if self._debug else ())
            self._buffer = GeometryBuffer(self.engine, W, H, planes)
        return self._buffer

    def record(self, push: _capi.Push, shard: Optional[_capi.Shard] = None) -> GeometryBuffer:
        gb = self._targets()
        st = self._settings.to_c()
        for fr in gb.to_c_split():
            if fr is not None:
                check(lib().vrt_render_geometry(self.engine.ctx, self._scene.handle, C.byref(push), C.byref(st), C.byref(fr),
                                                C.byref(shard) if shard is not None else None))
        return gb

    def record_rays(self, origins, dirs, resolution, frame=0) -> GeometryBuffer:
        """The G-buffer of a frame whose primary rays the caller supplies (vrt_render_rays): origins, dirs are float32 device
        tensors (W * H, 3), ray py * W + px for pixel (px, py) -- what RayCamera.rays returns.  The stage's own planes; of the
        debug planes color_f, hit_id, hit_voxel and hit_mask are filled; the count planes are not attached and are left untouched
        (zeros on a fresh stage, the last record()'s values on one that has drawn the built-in camera)."""
        torch = _torch()
        W, H = int(resolution[0]), int(resolution[1])
        if (W, H) != tuple(self._settings.renderResolution()):
            raise ValueError("record_rays: resolution must be the settings' renderResolution()")
        for t, what in ((origins, "origins"), (dirs, "dirs")):
            if not (torch.is_tensor(t) and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (W * H, 3)):
                raise ValueError(f"record_rays: {what} must be a contiguous float32 tensor of shape (W * H, 3)")
        gb = self._targets()
        st = self._settings.to_c()
        fr = gb.to_c(without=("steps_primary", "steps_total", "rays_total", "color8_strips"))
        check(lib().vrt_render_rays(self.engine.ctx, self._scene.handle, W, H, C.c_void_p(origins.data_ptr()), C.c_void_p(dirs.data_ptr()),
                                    int(frame) & 0xFFFFFFFF, C.byref(st), C.byref(fr)))
        return gb

    def prepare(self, shard: Optional[_capi.Shard] = None):
        """Frame loops whose settings do not change between frames: marshal the settings / target structs once and
        return launch(push) -> GeometryBuffer (a Python-side economy only; the same C-ABI call is made)."""
        gb = self._targets()
        st, fr, fr_diag = self._settings.to_c(), *gb.to_c_split()
        fn, ctx, scene = lib().vrt_render_geometry, self.engine.ctx, self._scene.handle
        pst, pfr = C.byref(st), C.byref(fr)
        psh = C.byref(shard) if shard is not None else None

        def launch(push: _capi.Push) -> GeometryBuffer:
            rc = fn(ctx, scene, C.byref(push), pst, pfr, psh)
            if rc == 0 and fr_diag is not None:
                rc = fn(ctx, scene, C.byref(push), pst, C.byref(fr_diag), psh)
            if rc != 0:
                check(rc)
            return gb
        launch._keepalive = (st, fr, fr_diag, shard, gb)
        return launch

    def prepare_batch(self, n: int, shard: Optional[_capi.Shard] = None, shards=None):
        """n frames per launch (vrt_render_geometry_batch): consecutive poses of an animation or the frames of a multi-GPU
        batch.  Returns launch(pushes) -> [GeometryBuffer] * n; every frame has its own planes, allocated here once.
        shards: one strip assignment per frame instead of one for all (vrt_render_geometry_slots)."""
        W, H = self._settings.renderResolution()
        planes = GBUFFER_PLANES + (DEBUG_PLANES if self._debug else ())
        gbs = [GeometryBuffer(self.engine, W, H, planes) for _ in range(int(n))]
        st = self._settings.to_c()
        split = [g.to_c_split() for g in gbs]
        frs = (_capi.Frame * int(n))(*[sp[0] for sp in split])
        frs_diag = (_capi.Frame * int(n))(*[sp[1] for sp in split]) if split and split[0][1] is not None else None
        arr = (_capi.Push * int(n))()
        fn, ctx, scene = lib().vrt_render_geometry_batch, self.engine.ctx, self._scene.handle
        pst = C.byref(st)
        psh = C.byref(shard) if shard is not None else None
        if shards is not None:
            if len(shards) != int(n):
                raise ValueError("prepare_batch: one shard per frame is required")
            shard = (_capi.Shard * int(n))(*shards)
            fn, psh = lib().vrt_render_geometry_slots, shard

        def launch(pushes, frames=None) -> list:
            """frames: another (_capi.Frame * n) table to render into (e.g. a copy of launch._keepalive[1] with other
            color8_strips pointers); default: the planes allocated above."""
            for k, p in enumerate(pushes):
                arr[k] = p
            rc = fn(ctx, scene, len(pushes), arr, pst, frs if frames is None else frames, psh)
            if rc == 0 and frs_diag is not None and frames is None:
                rc = fn(ctx, scene, len(pushes), arr, pst, frs_diag, psh)
            if rc != 0:
                check(rc)
            return gbs[:len(pushes)]
        launch._keepalive = (st, frs, arr, shard, gbs, frs_diag)
        return launch

    def record_batch(self, pushes, shard: Optional[_capi.Shard] = None) -> list:
        return self.prepare_batch(len(pushes), shard)(pushes)


class DenoiserStage:
    """DenoiserStage(engine, settings) / record(color, normal, pos) (denoiser_stage.cpp:22,156)."""

    def __init__(self, engine: Engine, settings: VoxelRenderSettings):
        self.engine, self._settings = engine, settings
        self._targets = None

    def record(self, colorInput, normalInput, posInput, shard: Optional[_capi.Shard] = None):
        torch = _torch()
        H, W = colorInput.shape[0], colorInput.shape[1]
        if self._targets is None or self._targets[0].shape != colorInput.shape:
            self._targets = [torch.zeros_like(colorInput), torch.zeros_like(colorInput)]     # _colorTargets ring
        ds = self._settings.denoiser_to_c()
        res = C.c_void_p()
        check(lib().vrt_denoise(self.engine.ctx, W, H, C.byref(ds), colorInput.data_ptr(), normalInput.data_ptr(),
                                posInput.data_ptr(), self._targets[0].data_ptr(), self._targets[1].data_ptr(),
                                C.byref(shard) if shard is not None else None, C.byref(res)))
        for t in self._targets:
            if t.data_ptr() == res.value:
                return t
        return colorInput

    def guard(self, pass_index: int) -> float:
        """Guard (RGBA8 codes) of weighted pass `pass_index` under the current settings (vrt_denoise_guard); inf: computed literally."""
        ds = self._settings.denoiser_to_c()
        g = C.c_float()
        check(lib().vrt_denoise_guard(C.byref(ds), int(pass_index), C.byref(g)))
        return float(g.value)

    def redone(self, pass_index: int) -> int:
        """Pixels of pass `pass_index` that the latest record() on this engine evaluated a second time, literally."""
        n = C.c_uint32()
        check(lib().vrt_debug_denoise_redone(self.engine.ctx, int(pass_index), C.byref(n)))
        return int(n.value)


class UpscalerStage:
    """UpscalerStage (upscaler_stage.cpp).  update() reproduces the jitter / frame sequence of :59-70 bit for bit
    (including the `frameCount > phaseCount` wrap, which lets frameCount reach phaseCount once per cycle).  The FSR2
    dispatch of record() (:72-161, a prebuilt third-party library) is out of scope; its stand-in is an exact N-frame
    accumulation of the jittered frames followed by the bilinear upscale to targetResolution (vrt_accumulate /
    vrt_resolve / vrt_blit), right while the camera stands still; under a moving camera record_reprojected() keeps the history
    by temporal reprojection (vrt_reproject) instead, at render resolution, and record_upsampled() keeps it at targetResolution
    (vrt_upsample): every jittered sample goes where it fell on the display grid, and no blit follows."""

    def __init__(self, engine: Engine, settings: VoxelRenderSettings):
        self.engine, self._settings = engine, settings
        self.reprojectSettings = ReprojectSettings()
        self.motion = None             # record_upsampled: motion vectors at targetResolution (RG32F)
        self._hist = None              # two (color16, surface) pairs, written in turn
        self._hist_cur = -1            # the pair the latest frame wrote; -1: no history
        self._prev_push = None
        self._prev_camera = None       # record_reprojected_camera: the previous frame's vrt_ray_camera
        self.jitterX = 0.0
        self.jitterY = 0.0
        self.frameCount = 0
        self._deltaMsec = 0.0
        self._accum = self._resolved = self._target = None
        self.accumulated = 0

    def phaseCount(self) -> int:
        return int(lib().vrt_jitter_phase_count(self._settings.renderResolution()[0], self._settings.targetResolution[0]))

    def update(self, delta: float):                                         # :59-70
        self._deltaMsec = delta * 1000
        phases = self.phaseCount()
        jx, jy = C.c_float(), C.c_float()
        check(lib().vrt_jitter_offset(self.frameCount % phases, phases, C.byref(jx), C.byref(jy)))
        self.jitterX, self.jitterY = jx.value, jy.value
        self.frameCount += 1
        if self.frameCount > phases:
            self.frameCount = 0

    def reset(self):
        """Drop the accumulated history (camera or scene changed)."""
        self.accumulated = 0
        self._hist_cur = -1

    # -- the history ring of the three temporal passes: two (color16, surface) pairs, written in turn

    def _ensure_histories(self, rows, cols, device, reset=False) -> bool:
        """The two pairs at rows x cols texels; they are new, and a new sequence starts, when their shape was another or on
        `reset`.  Returns whether that happened."""
        if reset or self._hist is None or self._hist[0][0].shape[:2] != (rows, cols):
            self._hist = [(_zeros((rows, cols, 4), "int16", device), _zeros((rows, cols, 4), "int32", device)) for _ in range(2)]
            self._hist_cur = -1
            return True
        return False

    def next_histories(self):
        """(history_in, history_out) of the next temporal call as vrt_history structs over the stage's own pairs; history_in is
        None when that call starts a sequence (the first one, after reset(), after a change of size)."""
        pair = lambda k: _capi.History(self._hist[k][0].data_ptr(), self._hist[k][1].data_ptr())
        return (pair(self._hist_cur), pair(1 - self._hist_cur)) if self._hist_cur >= 0 else (None, pair(0))

    def _commit(self, attr, block):
        """The call wrote history_out: it is the latest, and `block` the previous camera (kept as `attr`) of the next call."""
        self._hist_cur = 1 - self._hist_cur if self._hist_cur >= 0 else 0
        setattr(self, attr, type(block).from_buffer_copy(block))
        self.accumulated += 1

    def _ensure_target(self, device):
        TW, TH = self._settings.targetResolution
        self._target = _ensure(self._target, (TH, TW, 4), "uint8", device)

    def _ensure_reprojected(self, H, W, device):
        """What vrt_reproject and vrt_reproject_camera write: histories and the resolved image at render size, and the target."""
        if self._ensure_histories(H, W, device, reset=self._resolved is None or self._resolved.shape[:2] != (H, W)):
            self._resolved = _zeros((H, W, 4), "uint8", device)
            self._accum = None
        self._ensure_target(device)

    def _upscaled(self, W, H):
        """The resolved image, W x H, through the bilinear blit into the target."""
        TW, TH = self._settings.targetResolution
        check(lib().vrt_blit(self.engine.ctx, self._resolved.data_ptr(), W, H, self._target.data_ptr(), TW, TH))
        return self._target

    def record_reprojected(self, color, gbuffer: "GeometryBuffer", push: _capi.Push):
        """The temporal pass under a moving camera (vrt_reproject): `color` (normally the denoised image) is blended into the
        history fetched where each pixel's surface was on the previous frame's screen -- the frame recorded before this one, with
        the push it was given -- and the motion vectors are written into gbuffer.motion.  Two histories are written in turn;
        reset() starts a new sequence.  Returns the resolved image at targetResolution, like record()."""
        H, W = color.shape[0], color.shape[1]
        self._ensure_reprojected(H, W, color.device)
        hin, hout = self.next_histories()
        st = self.reprojectSettings.to_c(push)
        motion = gbuffer.planes.get("motion")
        check(lib().vrt_reproject(self.engine.ctx, W, H, C.byref(push), C.byref(self._prev_push if hin is not None else push), C.byref(st),
                                  color.data_ptr(), gbuffer.position.data_ptr(), gbuffer.normal.data_ptr(), _ref(hin), C.byref(hout),
                                  self._resolved.data_ptr(), motion.data_ptr() if motion is not None else None))
        self._commit("_prev_push", push)
        return self._upscaled(W, H)

    def record_reprojected_camera(self, color, gbuffer: "GeometryBuffer", ray_camera_c: _capi.RayCamera):
        """record_reprojected() for a frame drawn through a RayCamera (vrt_reproject_camera): ray_camera_c is the vrt_ray_camera
        block the frame's rays were made with (RayCamera.to_c(resolution, jitter)); the previous frame's is kept here, as
        record_reprojected() keeps the previous push.  One stage records through one of the two: their histories are the same
        buffers.  reprojectSettings.tolRel None is the camera model's default."""
        H, W = color.shape[0], color.shape[1]
        self._ensure_reprojected(H, W, color.device)
        if self._hist_cur >= 0 and (self._prev_camera is None or self._prev_camera.model != ray_camera_c.model):
            self._hist_cur = -1                                    # another camera model: a new sequence
        hin, hout = self.next_histories()
        st = _capi.ReprojectSettings()
        lib().vrt_reproject_camera_settings_default(C.byref(ray_camera_c), W, C.byref(st))
        self.reprojectSettings.over(st)
        motion = gbuffer.planes.get("motion")
        check(lib().vrt_reproject_camera(self.engine.ctx, W, H, C.byref(ray_camera_c), C.byref(self._prev_camera if hin is not None else ray_camera_c),
                                         C.byref(st), color.data_ptr(), gbuffer.position.data_ptr(), gbuffer.normal.data_ptr(), _ref(hin),
                                         C.byref(hout), self._resolved.data_ptr(), motion.data_ptr() if motion is not None else None))
        self._commit("_prev_camera", ray_camera_c)
        return self._upscaled(W, H)

    def record_upsampled(self, color, gbuffer: "GeometryBuffer", push: _capi.Push):
        """The temporal pass at display resolution (vrt_upsample): `color` (normally the denoised image, at render resolution)
        feeds a history pair at targetResolution, each sample where it fell on the display grid, the history fetched where each
        display pixel's surface was under the previous frame's camera.  The motion vectors, in display pixels, go into
        self.motion; gbuffer.motion is not touched.  reset() starts a new sequence.  Returns the resolved image at
        targetResolution -- there is no blit."""
        H, W = color.shape[0], color.shape[1]
        TW, TH = self._settings.targetResolution
        self._ensure_histories(TH, TW, color.device)
        self._ensure_target(color.device)
        self.motion = _ensure(self.motion, (TH, TW, 2), "float32", color.device)
        hin, hout = self.next_histories()
        st = self.reprojectSettings.to_c(push)
        check(lib().vrt_upsample(self.engine.ctx, W, H, TW, TH, C.byref(push), C.byref(self._prev_push if hin is not None else push), C.byref(st),
                                 color.data_ptr(), gbuffer.position.data_ptr(), gbuffer.normal.data_ptr(), _ref(hin), C.byref(hout),
                                 self._target.data_ptr(), self.motion.data_ptr()))
        self._commit("_prev_push", push)
        return self._target

    def record_upsampled_camera(self, color, gbuffer: "GeometryBuffer", ray_camera_c: _capi.RayCamera):
        """record_upsampled() for a frame drawn through a RayCamera (vrt_upsample_camera): ray_camera_c is the frame's camera
        WITHOUT sample offset and without jitter (RayCamera.to_c(resolution)); the samples' offsets went into the rays
        (RayCamera.rays(..., offset=) or, for the perspective model, jitter=).  The previous frame's camera is kept here, on the
        history ring, settings override and target of record_upsampled().  reprojectSettings.tolRel None is the camera model's
        default at the render width."""
        H, W = color.shape[0], color.shape[1]
        TW, TH = self._settings.targetResolution
        self._ensure_histories(TH, TW, color.device)
        self._ensure_target(color.device)
        self.motion = _ensure(self.motion, (TH, TW, 2), "float32", color.device)
        if self._hist_cur >= 0 and (self._prev_camera is None or self._prev_camera.model != ray_camera_c.model):
            self._hist_cur = -1                                    # another camera model: a new sequence
        hin, hout = self.next_histories()
        st = _capi.ReprojectSettings()
        lib().vrt_upsample_camera_settings_default(C.byref(ray_camera_c), W, C.byref(st))
        self.reprojectSettings.over(st)
        check(lib().vrt_upsample_camera(self.engine.ctx, W, H, TW, TH, C.byref(ray_camera_c),
                                        C.byref(self._prev_camera if hin is not None else ray_camera_c), C.byref(st), color.data_ptr(),
                                        gbuffer.position.data_ptr(), gbuffer.normal.data_ptr(), _ref(hin), C.byref(hout),
                                        self._target.data_ptr(), self.motion.data_ptr()))
        self._commit("_prev_camera", ray_camera_c)
        return self._target

    def history(self):
        """The latest history as (color16 uint16 [H, W, 4], surface uint32 [H, W, 4]) numpy arrays, or None."""
        if self._hist_cur < 0:
            return None
        c, s = self._hist[self._hist_cur]
        return c.cpu().numpy().view(np.uint16), s.cpu().numpy().view(np.uint32)

    def record(self, color):
        H, W = color.shape[0], color.shape[1]
        if self._accum is None or self._accum.shape[:2] != (H, W) or self._resolved.shape[:2] != (H, W):
            self._accum = _zeros((H, W, 4), "int32", color.device)
            self._resolved = _zeros((H, W, 4), "uint8", color.device)
            self.accumulated = 0
        self._ensure_target(color.device)
        check(lib().vrt_accumulate(self.engine.ctx, color.data_ptr(), self._accum.data_ptr(), W, H, 1 if self.accumulated == 0 else 0))
        self.accumulated += 1
        check(lib().vrt_resolve(self.engine.ctx, self._accum.data_ptr(), self._resolved.data_ptr(), W, H, self.accumulated))
        return self._upscaled(W, H)


class BlitStage:
    """BlitStage::record + shader/blit.frag (blit_stage.cpp:41-75): centre-cropped bilinear copy into a window-sized
    RGBA8 target (the swapchain image of the reference; here a device tensor)."""

    def __init__(self, engine: Engine, settings: VoxelRenderSettings):
        self.engine, self._settings = engine, settings
        self._target = None

    def record(self, source, windowSize):
        TW, TH = int(windowSize[0]), int(windowSize[1])
        self._target = _ensure(self._target, (TH, TW, 4), "uint8", source.device)
        check(lib().vrt_blit(self.engine.ctx, source.data_ptr(), source.shape[1], source.shape[0],
                             self._target.data_ptr(), TW, TH))
        return self._target


class VoxelRenderer:
    """VoxelRenderer (voxel_renderer.cpp:16-94): scene + camera + settings -> GeometryStage -> DenoiserStage ->
    UpscalerStage stand-in -> BlitStage -> RGBA8 image.  update() advances the camera and the jitter sequence as
    :33-39 does; until update() is called frame = 0 and cameraJitter = (0, 0).  GUI / swapchain are out of scope.

    temporal=False (default) keeps the frame graph at the hot path: the FSR branch of :86-87 is skipped and the
    image stays at renderResolution(); temporal=True takes that branch through the accumulation stand-in.
    windowSize=(w, h) appends the blit of :89.  reproject=True (with temporal=True) keeps the history under a moving camera:
    the temporal pass is UpscalerStage.record_reprojected instead of the pixel-by-pixel accumulation, and gBuffer.motion holds
    the motion vectors; reproject=False is the accumulation exactly.  upsample=True (with reproject=True) keeps that history at
    targetResolution instead (UpscalerStage.record_upsampled: no blit, display-resolution motion in upscaler.motion);
    upsample=False is the render-resolution path exactly.  camera=RayCamera(...): the G-buffer is drawn from that camera's rays
    (RayCamera.rays + GeometryStage.record_rays) instead of the built-in pinhole; the denoiser and the writers run unchanged.
    With temporal=True it needs reproject=True: the temporal pass is then UpscalerStage.record_reprojected_camera
    (vrt_reproject_camera) over the camera's to_c(resolution, jitter) of the frame, and gBuffer.motion holds its vectors; with
    upsample=True as well it is UpscalerStage.record_upsampled_camera (vrt_upsample_camera) at targetResolution: the perspective
    model keeps feeding the jitter sequence into camera_jitter (fov 90 is the pinhole path exactly), the orthographic and the
    panorama model take the same values as sample offsets (RayCamera.rays(..., offset=)), and the pass is handed the camera
    without either.  The accumulation (a moving ray camera has no pixel-wise history) is refused."""

    def __init__(self, engine: Engine, settings: Optional[VoxelRenderSettings] = None, scene: Optional[VoxelScene] = None,
                 noise=None, debug_planes: bool = False, temporal: bool = False, windowSize=None, reproject: bool = False,
                 upsample: bool = False, camera: Optional["RayCamera"] = None):
        if camera is not None and temporal and not reproject:
            raise ValueError("VoxelRenderer: temporal=True with a RayCamera needs reproject=True (the pixel-by-pixel accumulation is wrong for a moving ray camera)")
        if upsample and not reproject:
            raise ValueError("VoxelRenderer: upsample=True needs reproject=True (the display-resolution history is a reprojected one)")
        self.engine = engine
        self._settings = settings or VoxelRenderSettings()
        self._camera = CameraController()
        self.rayCamera = camera
        self._scene = scene if scene is not None else VoxelScene(engine, self._settings.voxPath)
        self._geometryStage = GeometryStage(engine, self._settings, self._scene, noise, debug_planes)
        self._denoiserStage = DenoiserStage(engine, self._settings)
        self._upscalerStage = UpscalerStage(engine, self._settings)
        self._blitStage = BlitStage(engine, self._settings)
        self.temporal = bool(temporal)
        self.reproject = bool(reproject)
        self.upsample = bool(upsample)
        self.windowSize = windowSize
        self._time = 0.0

    @property
    def settings(self):
        return self._settings

    @property
    def camera(self):
        return self._camera

    @property
    def scene(self):
        return self._scene

    @property
    def upscaler(self):
        return self._upscalerStage

    # frame / jitter live in the upscaler stage as in the reference (voxel_renderer.cpp:80-82)
    @property
    def frameCount(self):
        return self._upscalerStage.frameCount

    @frameCount.setter
    def frameCount(self, v):
        self._upscalerStage.frameCount = int(v)

    @property
    def jitter(self):
        return (self._upscalerStage.jitterX, self._upscalerStage.jitterY)

    @jitter.setter
    def jitter(self, v):
        self._upscalerStage.jitterX, self._upscalerStage.jitterY = float(v[0]), float(v[1])

    def update(self, delta: float, forward=0.0, strafe=0.0):          # :33-39
        self._time += delta
        self._camera.update(delta, forward, strafe)
        self._upscalerStage.update(delta)

    def push_constants(self) -> _capi.Push:                           # :72-83
        return make_push(self._camera, (self._scene.width, self._scene.height, self._scene.depth),
                         self._settings.renderResolution(), self.frameCount, self.jitter)

    def recordCommands(self, shard: Optional[_capi.Shard] = None):    # :55-94
        if self.upsample and shard is not None:
            raise ValueError("VoxelRenderer: upsampling across strips is not supported (include/vrt.h, vrt_upsample)")
        push = self.push_constants()
        if self.rayCamera is not None:
            if shard is not None:
                raise ValueError("VoxelRenderer: a RayCamera renders whole frames (vrt_render_rays has no vrt_shard)")
            res = self._settings.renderResolution()
            if self.upsample and self.rayCamera.model != _capi.CAMERA_PERSPECTIVE:
                # the jitter sequence as sample offsets: these two models apply no jitter
                origins, dirs = self.rayCamera.rays(self.engine, res, offset=self.jitter)
            else:
                origins, dirs = self.rayCamera.rays(self.engine, res, self.jitter)
            # (the display-resolution pass projects through the camera without offset and without jitter)
            ray_camera_c = self.rayCamera.to_c(res) if self.upsample else self.rayCamera.to_c(res, self.jitter)
            gBuffer = self._geometryStage.record_rays(origins, dirs, res, self.frameCount)
        else:
            gBuffer = self._geometryStage.record(push, shard)
        if self._settings.denoiserSettings.enable:
            color = self._denoiserStage.record(gBuffer.color, gBuffer.normal, gBuffer.position, shard)
        else:
            color = gBuffer.color
        self.gBuffer = gBuffer
        if self.temporal and self._settings.fsrSetttings.enable:      # :86-87
            if self.reproject:
                if shard is not None:
                    raise ValueError("VoxelRenderer: reprojection across strips is not supported (include/vrt.h, vrt_reproject)")
                if self.rayCamera is not None and self.upsample:
                    color = self._upscalerStage.record_upsampled_camera(color, gBuffer, ray_camera_c)
                elif self.rayCamera is not None:
                    color = self._upscalerStage.record_reprojected_camera(color, gBuffer, ray_camera_c)
                elif self.upsample:
                    color = self._upscalerStage.record_upsampled(color, gBuffer, push)
                else:
                    color = self._upscalerStage.record_reprojected(color, gBuffer, push)
            else:
                color = self._upscalerStage.record(color)
        if self.windowSize is not None:                               # :89
            color = self._blitStage.record(color, self.windowSize)
        return color

    render = recordCommands
